// C-ABI entry points of libcnerf_hip.so (declared in include/cnerf.h).  Host-side only: argument validation, buffer
// carving, launch sequencing on the caller's stream.  No allocation, no synchronisation, no global state -- with one exception, stated in
// the header: cnerf_render_rays_masked_forward reads the live counts of its compactions back and synchronises the stream for them.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cnerf_kernels.hpp"

using namespace cnerf;

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(CNERF_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// CNERF_F_NO_VOLUME: no feature volume, layer 0 reads the sample position
bool no_volume(const cnerf_cfg* c) { return (c->flags & CNERF_F_NO_VOLUME) != 0; }

int check_cfg(const cnerf_cfg* c, bool need_render) {
    if (!c) return fail(CNERF_EINVAL, "cfg is NULL");
    if (c->B < 1) return fail(CNERF_EINVAL, "B=%d must be >= 1", c->B);
    if (no_volume(c)) {
        if (c->C != 0 || c->n_levels != 0) return fail(CNERF_EINVAL, "CNERF_F_NO_VOLUME needs C = 0 and n_levels = 0 (C=%d, n_levels=%d)", c->C, c->n_levels);
        if (c->flags & CNERF_F_INPUT_XYZ) return fail(CNERF_EINVAL, "CNERF_F_NO_VOLUME and CNERF_F_INPUT_XYZ exclude each other");
        if (c->L >= 1 && c->layer_kind[0] == CNERF_LAYER_PFILM)
            return fail(CNERF_EINVAL, "CNERF_F_NO_VOLUME: per-point FiLM layers take their frequencies from a looked-up feature");
    } else if (c->C < 32 || c->C % 32 != 0 || c->C > 224) return fail(CNERF_EINVAL, "C=%d must be a multiple of 32 in [32,224]", c->C);
    if (c->n_levels < 0 || c->n_levels > CNERF_MAX_LEVELS) return fail(CNERF_EINVAL, "n_levels=%d out of range", c->n_levels);
    if (c->n_levels > 1 || (c->n_levels == 1 && (c->level_V[0] != c->V || c->level_C[0] != c->C))) {
        int sum = 0;
        for (int i = 0; i < c->n_levels; ++i) {
            if (c->level_V[i] < 2 || c->level_V[i] > 1024) return fail(CNERF_EINVAL, "level_V[%d]=%d out of range [2,1024]", i, c->level_V[i]);
            if (c->level_C[i] < 32 || c->level_C[i] % 32 != 0) return fail(CNERF_EINVAL, "level_C[%d]=%d must be a multiple of 32", i, c->level_C[i]);
            sum += c->level_C[i];
        }
        if (sum != c->C) return fail(CNERF_EINVAL, "sum of level_C (%d) != C (%d)", sum, c->C);
    }
    if (c->H != 64 && c->H != 128 && c->H != 256) return fail(CNERF_EINVAL, "H=%d must be 64, 128 or 256", c->H);
    if (!no_volume(c) && (c->V < 2 || c->V > 1024)) return fail(CNERF_EINVAL, "V=%d out of range [2,1024]", c->V);
    if (c->L < 1 || c->L > CNERF_MAX_LAYERS) return fail(CNERF_EINVAL, "L=%d out of range [1,%d]", c->L, CNERF_MAX_LAYERS);
    for (int l = 0; l < c->L; ++l) {
        const int k = c->layer_kind[l];
        if (k != CNERF_LAYER_FILM && k != CNERF_LAYER_SINE && k != CNERF_LAYER_RES && k != CNERF_LAYER_PFILM)
            return fail(CNERF_EINVAL, "layer_kind[%d]=%d unknown", l, k);
        if ((k == CNERF_LAYER_PFILM) != (c->layer_kind[0] == CNERF_LAYER_PFILM))
            return fail(CNERF_EINVAL, "per-point FiLM layers cannot be mixed with other layer kinds");
        if (l == 0 && k == CNERF_LAYER_RES) return fail(CNERF_EINVAL, "layer 0 cannot be a residual block");
    }
    if (!(c->voxel_length > 0.f)) return fail(CNERF_EINVAL, "voxel_length must be > 0");
    if (c->precision != CNERF_PREC_FP32 && c->precision != CNERF_PREC_FP16X3 && c->precision != CNERF_PREC_FP16)
        return fail(CNERF_EINVAL, "precision=%d unknown", c->precision);
    if (!(c->drop_p >= 0.0f && c->drop_p < 1.0f)) return fail(CNERF_EINVAL, "drop_p=%g out of [0,1)", (double)c->drop_p);
    if (c->drop_p > 0.0f && c->precision != CNERF_PREC_FP32) return fail(CNERF_EINVAL, "dropout (drop_p > 0) is implemented for precision fp32 only");
    if (need_render) {
        if (c->R < 1 || c->R > 4096) return fail(CNERF_EINVAL, "R=%d out of range [1,4096]", c->R);
        if (c->S < 2 || c->S > 128) return fail(CNERF_EINVAL, "S=%d out of range [2,128]", c->S);
        if (!(c->fov_deg > 0.0 && c->fov_deg < 180.0)) return fail(CNERF_EINVAL, "fov_deg out of (0,180)");
    }
    return CNERF_OK;
}

int n_levels_of(const cnerf_cfg* c) { return c->n_levels > 0 ? c->n_levels : (no_volume(c) ? 0 : 1); }
int level_V_of(const cnerf_cfg* c, int i) { return c->n_levels > 0 ? c->level_V[i] : c->V; }
int level_C_of(const cnerf_cfg* c, int i) { return c->n_levels > 0 ? c->level_C[i] : c->C; }
// floats of one image's volume level i (V^3 C, channel-last)
size_t level_floats(const cnerf_cfg* c, int i) { const size_t V = level_V_of(c, i); return V * V * V * level_C_of(c, i); }

// What every host path derives from the cfg's layer list, computed here only
struct NetCounts {
    int n_mats;             // weight matrices before the head (a residual block: fc1 and fc2)
    int n_film;             // FiLM layers: rows of freq / phase per image
    int n_drop;             // layers whose output dropout masks (all but residual blocks)
    int n_in;               // 32-wide input tiles of layer 0
    int k0;                 // real input width of layer 0
    float drop_scale;       // ATen: noise.bernoulli_(1 - p).div_(1 - p): the factor is 1 / float(1 - p) in fp32
    uint32_t drop_thresh;   // a keep draw below p 2^32 drops
};
NetCounts counts_of(const cnerf_cfg* c) {
    NetCounts n{0, 0, 0, 1, 3, 0.0f, 0u};
    for (int l = 0; l < c->L; ++l) {
        n.n_mats += c->layer_kind[l] == CNERF_LAYER_RES ? 2 : 1;
        n.n_film += c->layer_kind[l] == CNERF_LAYER_FILM;
        n.n_drop += c->layer_kind[l] != CNERF_LAYER_RES;
    }
    if (c->layer_kind[0] != CNERF_LAYER_PFILM && !no_volume(c)) {      // (per-point FiLM, no volume: layer 0 reads the sample position)
        n.n_in = c->C / 32 + ((c->flags & CNERF_F_INPUT_XYZ) ? 1 : 0);
        n.k0 = c->C + ((c->flags & CNERF_F_INPUT_XYZ) ? 3 : 0);
    }
    n.drop_scale = 1.0f / (float)(1.0 - (double)c->drop_p);
    const double th = (double)c->drop_p * 4294967296.0 + 0.5;
    n.drop_thresh = th >= 4294967295.0 ? 0xffffffffu : (uint32_t)th;
    return n;
}

// The packed buffer of cnerf_pack_field, offsets in floats from its start:
//   [weight stream][biases][head bias (4)][fp16 precisions: 1/S, max|W| slots][ones H][zeros H]
// weight stream: the matrices in consumption order, fp32 float4 tiles or fp16 fragments (field_kernel.hip, field_h3.hip, field_pw16.hip).
// biases: FiLM / plain-sine / residual: one per matrix in order (a residual block: b1 then b2); per-point FiLM: mapping b1 (256), then per
// layer b, freq bias, phase bias.  Per-point FiLM in fp16: the biases, the head bias and pw16_consts_kernel's constants are all written
// by that kernel.  ones / zeros: a plain sine layer runs as a FiLM layer with freq = 1, phase = 0.
struct PackedLayout {
    size_t tile_floats;     // one 32-row output tile against one 32-wide input tile
    size_t weight_floats;   // = the offset of the biases
    size_t head_bias;
    size_t pw_consts;       // per-point FiLM fp16: the scalar constants of pw16_consts_kernel (2 + 4 L, padded to 4)
    size_t inv_s, wmax;     // fp16 precisions: n_slots 1/S, then n_slots max|W| scratch words (together padded to 4)
    int n_slots;
    size_t ones, zeros;
    size_t total;
    // floats one packed matrix of n_out rows and K inputs moves the write pointer
    size_t mat_floats(int n_out, int K) const { return (size_t)((n_out + 31) / 32) * ((K + 31) / 32) * tile_floats; }
};

PackedLayout packed_layout(const cnerf_cfg* c) {
    const NetCounts n = counts_of(c);
    const int H = c->H, L = c->L;
    const bool pfilm = c->layer_kind[0] == CNERF_LAYER_PFILM, half = c->precision != CNERF_PREC_FP32;
    PackedLayout p{};
    // fp32: 4 x 64 lanes x float4; fp16: two k-chunks of 16 x 64 lanes x 8 fp16 per part (fp16x3: two parts)
    p.tile_floats = half ? (c->precision == CNERF_PREC_FP16 ? 1 : 2) * 2 * 64 * 8 / 2 : 4 * 64 * 4;
    if (pfilm) {   // Wm1 | per layer: W_l, freq rows, phase rows (fp16: interleaved per output tile) | head
        p.weight_floats = p.mat_floats(256, 32) + p.mat_floats(4, H);     // (a single 32-channel volume)
        for (int l = 0; l < L; ++l) p.weight_floats += p.mat_floats(H, l == 0 ? 3 : H) + 2 * p.mat_floats(H, 256);
        p.head_bias = p.weight_floats + 256 + 3 * (size_t)L * H;
        p.pw_consts = p.head_bias + 4;
        p.n_slots = 3 * L + 2;
        p.inv_s = half ? p.pw_consts + (2 + 4 * (size_t)L + 3) / 4 * 4 : p.pw_consts;
    } else {
        p.weight_floats = p.mat_floats(4, H);   // head, one 32-row tile
        for (int m = 0; m < n.n_mats; ++m) p.weight_floats += p.mat_floats(H, m == 0 ? n.k0 : H);
        p.head_bias = p.weight_floats + (size_t)n.n_mats * H;
        p.n_slots = n.n_mats + 1;
        p.inv_s = p.head_bias + 4;
    }
    p.wmax = p.inv_s + p.n_slots;
    p.ones = half ? p.inv_s + (2 * (size_t)p.n_slots + 3) / 4 * 4 : p.inv_s;
    p.zeros = p.ones + H;
    p.total = p.zeros + H;
    return p;
}

PhiloxKey philox_of(const cnerf_cfg* c) {
    return PhiloxKey{c->philox ? 1u : 0u, c->philox_offset, (uint32_t)(c->philox_seed & 0xffffffffull), (uint32_t)(c->philox_seed >> 32)};
}

RayGeom make_geom(const cnerf_cfg* c) {
    RayGeom g;
    g.R = c->R;
    g.S = c->S;
    // z = ones(float32) / np.tan((2*pi*fov/360)/2): the double tangent is rounded to fp32, then 1/x in fp32
    g.focal = 1.0f / (float)tan((2.0 * M_PI * c->fov_deg / 360.0) / 2.0);
    g.ray_start = c->ray_start;
    g.ray_end = c->ray_end;
    return g;
}

// image0: first image of the sub-range this launch works on (per-image pointers are offset here)
int fill_field_args(FieldArgs& a, const cnerf_cfg* c, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols,
                    const float* packed, const float* freq, const float* phase, int image0 = 0) {
    memset(&a, 0, sizeof(a));
    const PackedLayout pl = packed_layout(c);
    const NetCounts nc = counts_of(c);
    if (!vols && !no_volume(c)) return fail(CNERF_EINVAL, "volumes are NULL");
    int tk = 0;
    for (int i = 0; i < n_levels_of(c); ++i) {
        const int C = level_C_of(c, i);
        if (!vols->level[i]) return fail(CNERF_EINVAL, "volume level %d is NULL", i);
        const size_t per_image = level_floats(c, i);
        a.lvl_vol[i] = vols->level[i] + (size_t)image0 * per_image;
        a.lvl_grad[i] = (gvols && gvols->level[i]) ? gvols->level[i] + (size_t)image0 * per_image : nullptr;
        a.lvl_V[i] = level_V_of(c, i);
        a.lvl_C[i] = C;
        for (int cc = 0; cc < C; cc += 32, ++tk) {
            if (tk >= 8) return fail(CNERF_EINVAL, "more than 8 input tiles");
            a.in_level[tk] = i;
            a.in_chan[tk] = cc;
        }
    }
    if (c->flags & (CNERF_F_INPUT_XYZ | CNERF_F_NO_VOLUME)) {      // (no volume: the xyz tile is the only one)
        if (tk >= 8) return fail(CNERF_EINVAL, "more than 8 input tiles");
        a.in_level[tk] = -1;
        a.in_chan[tk] = 0;
        ++tk;
    }
    a.n_in = tk;
    freq = (nc.n_film && freq) ? freq + (size_t)image0 * nc.n_film * c->H : freq;
    phase = (nc.n_film && phase) ? phase + (size_t)image0 * nc.n_film * c->H : phase;
    a.packed = packed;
    a.bias = packed ? packed + pl.weight_floats : nullptr;      // (cnerf_scatter_patches has no weights)
    a.freq = nc.n_film ? freq : nullptr;
    a.phase = nc.n_film ? phase : nullptr;
    a.film_stride = nc.n_film * c->H;
    a.bias_floats = (int)(pl.ones - pl.weight_floats);
    a.geom = make_geom(c);
    a.half_voxel = c->voxel_length / 2.0f;
    a.L = c->L;
    a.n_mats = nc.n_mats;
    a.flags = c->flags;
    for (int l = 0; l < c->L; ++l) a.layer_kind[l] = c->layer_kind[l];
    a.philox = philox_of(c);
    a.image0 = image0;
    if (c->drop_p > 0.0f) {
        a.drop_scale = nc.drop_scale;
        a.drop_thresh = nc.drop_thresh;
        a.n_drop = nc.n_drop;
    }
    return CNERF_OK;
}

// which keep decisions a pass uses: the injected bytes, or Philox stream `stream_id` (fill_field_args set the rest)
void set_dropout(FieldArgs& a, const cnerf_cfg* c, const uint8_t* mask, uint32_t stream_id, long long n_per_image) {
    a.drop_mask = c->drop_p > 0.0f ? mask : nullptr;
    a.drop_stream = stream_id;
    a.drop_points = (long long)c->B * n_per_image;
}

hipError_t launch_forward(const FieldArgs& a, const cnerf_cfg* c, hipStream_t stream) {
    if (c->layer_kind[0] == CNERF_LAYER_PFILM && c->precision != CNERF_PREC_FP32)
        return c->precision == CNERF_PREC_FP16 ? launch_field_pw1(a, c->H, stream) : launch_field_pw3(a, c->H, stream);
    if (c->precision == CNERF_PREC_FP16X3) return launch_field_h3(a, c->H, stream);
    if (c->precision == CNERF_PREC_FP16) return launch_field_h1(a, c->H, stream);
    return launch_field(a, c->H, stream);
}

void set_points(FieldArgs& a, int B, long long n_per_image) {
    a.n_per_image = n_per_image;
    a.tiles_per_image = (n_per_image + 31) / 32;
    a.total_tiles = a.tiles_per_image * B;
}

// FieldArgs of one field pass over images [image0, image0 + n_images) of the call: pass 0 = coarse samples (u_strat or NULL),
// 1 = fine samples (fine_z), 2 = explicit points (B, R*R*S, 3) carried in u_strat.  The per-image inputs are the call's full tensors.
int pass_args(FieldArgs& a, const cnerf_cfg* c, int pass, int image0, int n_images, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols,
              const float* packed, const float* freq, const float* phase, const float* cam2world, const float* u_strat, const float* fine_z) {
    if (int rc = fill_field_args(a, c, vols, gvols, packed, freq, phase, image0)) return rc;
    const long long npi = (long long)c->R * c->R * c->S;
    set_points(a, n_images, npi);
    a.cam2world = cam2world + (size_t)image0 * 16;
    if (pass == 0) {
        a.mode = FIELD_MODE_COARSE;
        a.u_strat = u_strat ? u_strat + (size_t)image0 * npi : nullptr;
    } else if (pass == 1) {
        a.mode = FIELD_MODE_FINE;
        a.fine_z = fine_z + (size_t)image0 * npi;
    } else {
        if (!u_strat) return fail(CNERF_EINVAL, "field_backward: pass 2 takes the points (B,R*R*S,3) in the u_strat argument");
        a.mode = FIELD_MODE_POINTS;
        a.points = u_strat + (size_t)image0 * npi * 3;
    }
    return CNERF_OK;
}

// FieldArgs of explicit points: n_images images from image0 of the call, n_per_image positions each (`points`: the first image's), the
// keep decisions of dropout stream PHILOX_DROP_POINTS (`mask`, or Philox when NULL)
int points_args(FieldArgs& a, const cnerf_cfg* c, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols, const float* packed, const float* freq,
                const float* phase, const float* points, int image0, int n_images, long long n_per_image, const uint8_t* mask) {
    if (int rc = fill_field_args(a, c, vols, gvols, packed, freq, phase, image0)) return rc;
    a.mode = FIELD_MODE_POINTS;
    a.points = points;
    set_points(a, n_images, n_per_image);
    set_dropout(a, c, mask, PHILOX_DROP_POINTS, n_per_image);
    return CNERF_OK;
}

int check_grad_vols(const cnerf_cfg* c, const cnerf_grad_volumes* g, const char* who) {
    for (int i = 0; i < n_levels_of(c); ++i)
        if (!g->level[i]) return fail(CNERF_EINVAL, "%s: gradient volume %d is NULL", who, i);
    return CNERF_OK;
}

// PointsGradArgs of image b's volume levels and n points; the caller sets the gradient rows it reads (gfeat / gxyz)
PointsGradArgs points_grad_args(const cnerf_cfg* c, const cnerf_volumes* vols, int b, const float* points, float* grad_points, long long n) {
    PointsGradArgs pg{};
    pg.n_levels = n_levels_of(c);
    for (int i = 0; i < pg.n_levels; ++i) {
        pg.lvl_vol[i] = vols->level[i] + (size_t)b * level_floats(c, i);
        pg.lvl_V[i] = level_V_of(c, i);
        pg.lvl_C[i] = level_C_of(c, i);
    }
    pg.points = points;
    pg.grad_points = grad_points;
    pg.n = n;
    pg.half_voxel = c->voxel_length / 2.0f;
    return pg;
}

// the draws of a call that passes no cnerf_rng: none
const cnerf_rng* rng_or_none(const cnerf_rng* rng) {
    static const cnerf_rng no_rng = {};
    return rng ? rng : &no_rng;
}

// The matrices of a FiLM / plain-sine / residual network in slab order (a residual block: fc1, fc2), their kinds and gradient buffers
// (NULL without G)
struct MatrixSet {
    const float *W[2 * CNERF_MAX_LAYERS], *b[2 * CNERF_MAX_LAYERS];
    float *dW[2 * CNERF_MAX_LAYERS], *db[2 * CNERF_MAX_LAYERS];
    int film_of[2 * CNERF_MAX_LAYERS];
    int H, film_stride;
    // matrix m's slice of freq / grad_freq / grad_phase for the chunk from image b0 (NULL unless m is a FiLM matrix)
    const float* film(const float* t, int m, int b0) const { return film_of[m] >= 0 ? t + (size_t)b0 * film_stride + (size_t)film_of[m] * H : nullptr; }
    float* film(float* t, int m, int b0) const { return film_of[m] >= 0 ? t + (size_t)b0 * film_stride + (size_t)film_of[m] * H : nullptr; }
};
int matrix_set(const cnerf_cfg* cfg, const cnerf_field_params* P, const cnerf_field_param_grads* G, const char* who, MatrixSet& ms) {
    int nm = 0, nfilm = 0;
    for (int l = 0; l < cfg->L; ++l) {
        const bool res = cfg->layer_kind[l] == CNERF_LAYER_RES;
        if (!P->w[l] || !P->b[l] || (res && (!P->w2[l] || !P->b2[l]))) return fail(CNERF_EINVAL, "%s: parameters of layer %d are NULL", who, l);
        ms.W[nm] = P->w[l]; ms.b[nm] = P->b[l]; ms.dW[nm] = G ? G->w[l] : nullptr; ms.db[nm] = G ? G->b[l] : nullptr;
        ms.film_of[nm] = cfg->layer_kind[l] == CNERF_LAYER_FILM ? nfilm++ : -1;
        ++nm;
        if (res) {
            ms.W[nm] = P->w2[l]; ms.b[nm] = P->b2[l]; ms.dW[nm] = G ? G->w2[l] : nullptr; ms.db[nm] = G ? G->b2[l] : nullptr;
            ms.film_of[nm] = -1;
            ++nm;
        }
    }
    ms.H = cfg->H;
    ms.film_stride = counts_of(cfg).n_film * cfg->H;
    return CNERF_OK;
}

// Workspace of cnerf_render_forward, carved in this order (every piece 256-byte aligned): the coarse and fine rgb_sigma (N, 4) and z (N),
// then the weight folding.  fp32: the folded FiLM constants (4 per image, matrix and channel) and the row-scaled per-image copies of the
// layer weights (WFOLD, field_kernel.hip).  fp16 precisions, in the same place: the per-image copies of the whole packed weight stream,
// their constants K S' / 1 / S' and the row multipliers (field_h3.hip, "weight folding per image").  The per-point FiLM family computes
// its frequencies per point and folds nothing, yet reserves the fp32 regions.
struct ForwardLayout {
    size_t c_rs, f_rs, c_z, f_z;
    size_t fold, packed_img;            // fp32
    long long layer_floats;             // fp32: one image's copy of the layer weights
    size_t img16, fold16, rowf;         // fp16 precisions
    size_t total;
};
ForwardLayout forward_layout(const cnerf_cfg* c) {
    const PackedLayout pl = packed_layout(c);
    const NetCounts nc = counts_of(c);
    const size_t N = (size_t)c->B * c->R * c->R * c->S, B = c->B, H = c->H, NT = H / 32, mats = nc.n_mats;
    ForwardLayout F{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    F.c_rs = take(N * 4 * sizeof(float));
    F.f_rs = take(N * 4 * sizeof(float));
    F.c_z = take(N * sizeof(float));
    F.f_z = take(N * sizeof(float));
    if (c->precision != CNERF_PREC_FP32 && c->layer_kind[0] != CNERF_LAYER_PFILM) {
        F.img16 = take(B * pl.weight_floats * sizeof(float));
        F.fold16 = take(B * mats * (H + 1) * sizeof(float));
        F.rowf = take(B * mats * H * sizeof(float));
    } else {
        F.layer_floats = (long long)((NT * nc.n_in + (mats - 1) * NT * NT) * 1024);
        F.fold = take(4 * B * mats * H * sizeof(float));
        F.packed_img = take(B * (size_t)F.layer_floats * sizeof(float));
    }
    F.total = off;
    return F;
}

// the activation-storing re-run of a half-precision backward: the pass `a` again, storing fp16 TB16 activations (amax: per-point FiLM
// family only); its head output goes to `scratch`, (n,4) floats nobody reads -- the chain overwrites that buffer entirely
FieldArgs storing_args(const FieldArgs& a, long long n_points, void* feat, void* h, void* c, float* amax, void* scratch) {
    FieldArgs s = a;
    s.rgb_sigma = (float*)scratch;
    s.act_points = n_points;
    s.act_feat = (float*)feat;
    s.act_h = (float*)h;
    s.act_c = (float*)c;
    s.act_amax = amax;
    s.act_tb16 = 1;
    return s;
}

// The exact fp32 backward of one field pass `fa` (n_points rows, gradient volumes and dropout set): the activation-storing re-run
// in cfg->precision (`packed` is in that precision's layout), then the fp32 gradient chain on the transposed fp32 weights, which
// scatters d(feature volume) itself.  grad_out / saved_out: the rows of this launch.
int field_backward_run(FieldArgs fa, const cnerf_cfg* cfg, long long n_points, const float* packed_t, const float* grad_out, const float* saved_out,
                       float* act_feat, float* act_h, float* act_c, float* act_g, float* act_go, hipStream_t stream) {
    fa.rgb_sigma = act_go;          // the re-run forward needs somewhere to put its head output: overwritten below by go'
    fa.act_points = n_points;
    fa.act_feat = act_feat;
    fa.act_h = act_h;
    fa.act_c = act_c;
    if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, "field kernel (activation store)");
    fa.packed_t = packed_t;
    fa.grad_out = grad_out;
    fa.saved_out = saved_out;
    fa.act_g = act_g;
    fa.act_go = act_go;
    if (hipError_t e = launch_field_backward(fa, cfg->H, stream)) return hip_fail(e, "field backward kernel");
    return CNERF_OK;
}

}  // namespace

extern "C" {

int cnerf_abi_version(void) { return CNERF_ABI_VERSION; }

const char* cnerf_last_error(void) { return g_err; }

int cnerf_philox_fill(uint64_t seed, uint32_t offset, uint32_t stream_id, int64_t n, int32_t normal, float* out, void* stream) {
    g_err[0] = 0;
    if (!out || n < 1 || stream_id > 3) return fail(CNERF_EINVAL, "philox_fill: bad argument (stream_id 0..3)");
    const PhiloxKey k{1u, offset, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32)};
    if (hipError_t e = launch_philox_fill(k, stream_id, (long long)n, normal, out, (hipStream_t)stream)) return hip_fail(e, "philox_fill");
    return CNERF_OK;
}

int cnerf_workspace_bytes(const cnerf_cfg* cfg, size_t* packed, size_t* fvol_cl, size_t* fwd_ws) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, fwd_ws != nullptr)) return rc;
    if (packed) *packed = align256(packed_layout(cfg).total * sizeof(float));
    if (fvol_cl) {   // all levels together
        size_t fl = 0;
        for (int i = 0; i < n_levels_of(cfg); ++i) fl += (size_t)cfg->B * level_floats(cfg, i);
        *fvol_cl = align256(fl * sizeof(float));
    }
    if (fwd_ws) *fwd_ws = forward_layout(cfg).total;
    return CNERF_OK;
}

int cnerf_fvol_channel_last(int32_t B, int32_t C, int32_t V, const float* fvol_cf, float* fvol_cl, void* stream) {
    g_err[0] = 0;
    if (B < 1 || V < 1 || C < 32 || C % 32 || !fvol_cf || !fvol_cl) return fail(CNERF_EINVAL, "fvol_channel_last: bad argument (C must be a multiple of 32)");
    if (hipError_t e = launch_transpose_cl(B, C, V, fvol_cf, fvol_cl, true, (hipStream_t)stream)) return hip_fail(e, "transpose");
    return CNERF_OK;
}

int cnerf_fvol_channel_first(int32_t B, int32_t C, int32_t V, const float* fvol_cl, float* fvol_cf, void* stream) {
    g_err[0] = 0;
    if (B < 1 || V < 1 || C < 32 || C % 32 || !fvol_cf || !fvol_cl) return fail(CNERF_EINVAL, "fvol_channel_first: bad argument (C must be a multiple of 32)");
    if (hipError_t e = launch_transpose_cl(B, C, V, fvol_cl, fvol_cf, false, (hipStream_t)stream)) return hip_fail(e, "transpose");
    return CNERF_OK;
}

int cnerf_pack_field(const cnerf_cfg* cfg, const cnerf_field_params* p, float* packed, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (!p || !packed) return fail(CNERF_EINVAL, "pack_field: NULL argument");
    // every parameter is checked before the first launch is queued
    const bool pfilm = cfg->layer_kind[0] == CNERF_LAYER_PFILM, half = cfg->precision != CNERF_PREC_FP32;
    MatrixSet ms;
    if (pfilm) {
        if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "per-point FiLM: a single 32-channel feature volume is supported");
        if (!p->map_w1 || !p->map_b1 || !p->map_w2 || !p->map_b2 || !p->w_final || !p->b_final)
            return fail(CNERF_EINVAL, "pack_field: mapping network / head is NULL");
        for (int l = 0; l < cfg->L; ++l)
            if (!p->w[l] || !p->b[l]) return fail(CNERF_EINVAL, "pack_field: layer %d weight/bias is NULL", l);
    } else {
        if (int rc = matrix_set(cfg, p, nullptr, "pack_field", ms)) return rc;
        if (!p->w_final || !p->b_final) return fail(CNERF_EINVAL, "pack_field: head is NULL");
    }
    hipStream_t stream = (hipStream_t)stream_;
    const PackedLayout pl = packed_layout(cfg);
    const NetCounts nc = counts_of(cfg);
    const int H = cfg->H, NT = H / 32, L = cfg->L;
    const size_t LH = (size_t)L * H;
    auto pack16 = cfg->precision == CNERF_PREC_FP16 ? launch_pack_h1 : launch_pack_h3;
    const char* packer = half ? "pack_h3" : "pack_matrix";
    float* wdst = packed;
    float* inv_s = packed + pl.inv_s;
    float* wmax = packed + pl.wmax;
    float* bdst = packed + pl.weight_floats;
    auto copy = [&](const float* src, size_t n) {          // the next n bias floats
        const hipError_t e = hipMemcpyAsync(bdst, src, n * sizeof(float), hipMemcpyDeviceToDevice, stream);
        bdst += n;
        return e ? hip_fail(e, "bias copy") : CNERF_OK;
    };
    if (pfilm && half) {      // field_pw16.hip; pw16_consts_kernel writes the biases and constants
        // slots of 1/S and max|W|: [Wm1 | per layer: W_l, freq rows, phase rows | head]; the layer matrices interleaved per output tile
        const size_t big = pl.mat_floats(32, 256), small = pl.mat_floats(32, H);       // one output tile of a freq / phase and a W_l matrix
        if (hipError_t e = pack16(p->map_w1, 256, cfg->C, 8, true, wdst, inv_s, wmax, stream, 0)) return hip_fail(e, packer);
        wdst += pl.mat_floats(256, cfg->C);
        if (hipError_t e = pack16(p->w[0], H, 3, NT, true, wdst, inv_s + 1, wmax + 1, stream, 0)) return hip_fail(e, packer);
        wdst += pl.mat_floats(H, 3);
        for (int l = 0; l < L; ++l) {
            // the tiles of the layer's three matrices interleaved per output tile: [freq rows t | W_l t (l >= 1) | phase rows t]
            const long long t_stride = 16 + 16 + (l ? 2 * NT : 0);          // fragment pairs (one per k-chunk) per output tile
            const float* wf = p->map_w2 + (size_t)l * H * 256;
            const float* wp = p->map_w2 + (LH + (size_t)l * H) * 256;
            float* d = wdst;
            if (hipError_t e = pack16(wf, H, 256, NT, false, d, inv_s + 2 + 3 * l, wmax + 2 + 3 * l, stream, t_stride)) return hip_fail(e, packer);
            d += big;
            if (l) {
                if (hipError_t e = pack16(p->w[l], H, H, NT, false, d, inv_s + 1 + 3 * l, wmax + 1 + 3 * l, stream, t_stride)) return hip_fail(e, packer);
                d += small;
            }
            if (hipError_t e = pack16(wp, H, 256, NT, false, d, inv_s + 3 + 3 * l, wmax + 3 + 3 * l, stream, t_stride)) return hip_fail(e, packer);
            wdst += (size_t)NT * (2 * big + (l ? small : 0));
        }
        if (hipError_t e = pack16(p->w_final, 4, H, 1, false, wdst, inv_s + 3 * L + 1, wmax + 3 * L + 1, stream, 0)) return hip_fail(e, packer);
        if (hipError_t e = launch_pw16_consts(p, L, H, inv_s, bdst, stream)) return hip_fail(e, "pw16_consts");
        return CNERF_OK;
    }
    if (pfilm) {              // fp32: mapping hidden | per layer (main, freq rows, phase rows) | head
        if (hipError_t e = launch_pack_matrix(p->map_w1, 256, cfg->C, 8, wdst, stream)) return hip_fail(e, packer);
        wdst += pl.mat_floats(256, cfg->C);
        if (int rc = copy(p->map_b1, 256)) return rc;
        for (int l = 0; l < L; ++l) {
            const int K = (l == 0) ? 3 : H;
            if (hipError_t e = launch_pack_matrix(p->w[l], H, K, NT, wdst, stream)) return hip_fail(e, packer);
            wdst += pl.mat_floats(H, K);
            if (hipError_t e = launch_pack_matrix(p->map_w2 + (size_t)l * H * 256, H, 256, NT, wdst, stream)) return hip_fail(e, packer);
            wdst += pl.mat_floats(H, 256);
            if (hipError_t e = launch_pack_matrix(p->map_w2 + (LH + (size_t)l * H) * 256, H, 256, NT, wdst, stream)) return hip_fail(e, packer);
            wdst += pl.mat_floats(H, 256);
            if (int rc = copy(p->b[l], H)) return rc;
            if (int rc = copy(p->map_b2 + (size_t)l * H, H)) return rc;
            if (int rc = copy(p->map_b2 + LH + (size_t)l * H, H)) return rc;
        }
    } else {                  // FiLM / plain-sine / residual: every matrix in slab order, then the head (one 32-row tile)
        for (int m = 0; m < nc.n_mats; ++m) {
            const int K = m == 0 ? nc.k0 : H;                  // layer 0: C (+3), zero padded to 32 * n_in columns
            if (hipError_t e = half ? pack16(ms.W[m], H, K, NT, m == 0, wdst, inv_s + m, wmax + m, stream, 0)
                                    : launch_pack_matrix(ms.W[m], H, K, NT, wdst, stream))
                return hip_fail(e, packer);
            wdst += pl.mat_floats(H, K);
            if (int rc = copy(ms.b[m], H)) return rc;
        }
    }
    if (hipError_t e = half ? pack16(p->w_final, 4, H, 1, false, wdst, inv_s + nc.n_mats, wmax + nc.n_mats, stream, 0)
                            : launch_pack_head(p->w_final, H, wdst, stream))
        return hip_fail(e, packer);
    if (int rc = copy(p->b_final, 4)) return rc;
    if (hipError_t e = launch_fill(packed + pl.ones, 1.0f, H, stream)) return hip_fail(e, "fill");
    if (hipError_t e = launch_fill(packed + pl.zeros, 0.0f, H, stream)) return hip_fail(e, "fill");
    return CNERF_OK;
}

int cnerf_gather_features(const cnerf_cfg* cfg, const float* fvol_cl, const float* points, int64_t n_per_image,
                          float* feat, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (no_volume(cfg)) return fail(CNERF_EINVAL, "gather_features: CNERF_F_NO_VOLUME networks look nothing up");
    if (!fvol_cl || !points || !feat || n_per_image < 1) return fail(CNERF_EINVAL, "gather_features: bad argument");
    if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "gather_features: single 32-channel volume only");
    GatherArgs a{fvol_cl, points, feat, (long long)n_per_image, cfg->B, cfg->V, cfg->C, cfg->voxel_length / 2.0f};
    if (hipError_t e = launch_gather(a, (hipStream_t)stream)) return hip_fail(e, "gather");
    return CNERF_OK;
}

int cnerf_weight_grad(int32_t n_images, int64_t n_per_image, int32_t H, int32_t K, const float* g_arg, const float* x, float* dW,
                      float* colsum, void* stream) {
    g_err[0] = 0;
    if (!g_arg || !x || !dW || !colsum) return fail(CNERF_EINVAL, "weight_grad: NULL argument");
    if (n_images < 1 || n_per_image < 1) return fail(CNERF_EINVAL, "weight_grad: empty chunk");
    if ((H != 64 && H != 128 && H != 256) || K < 32 || K > 256 || K % 32)
        return fail(CNERF_EINVAL, "weight_grad: H=%d must be 64/128/256 and K=%d a multiple of 32 up to 256", H, K);
    if (hipError_t e = launch_weight_grad(n_images, n_per_image, H, K, g_arg, x, dW, colsum, (hipStream_t)stream))
        return hip_fail(e, "weight_grad");
    return CNERF_OK;
}

int cnerf_scatter_features(const cnerf_cfg* cfg, const float* points, int64_t n_per_image, const float* grad_feat,
                           float* grad_fvol_cl, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (no_volume(cfg)) return fail(CNERF_EINVAL, "scatter_features: CNERF_F_NO_VOLUME networks have no volume to scatter into");
    if (!grad_fvol_cl || !points || !grad_feat || n_per_image < 1) return fail(CNERF_EINVAL, "scatter_features: bad argument");
    if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "scatter_features: single 32-channel volume only");
    GatherArgs a{nullptr, points, nullptr, (long long)n_per_image, cfg->B, cfg->V, cfg->C, cfg->voxel_length / 2.0f};
    if (hipError_t e = launch_scatter(a, grad_feat, grad_fvol_cl, (hipStream_t)stream)) return hip_fail(e, "scatter");
    return CNERF_OK;
}

int cnerf_field_forward(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* freq,
                        const float* phase, const float* points, int64_t n_per_image, float* rgb_sigma, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if ((!vols && !no_volume(cfg)) || !packed || !points || !rgb_sigma || n_per_image < 1) return fail(CNERF_EINVAL, "field_forward: bad argument");
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "field_forward: FiLM layers need freq and phase");
    FieldArgs a;
    if (int rc = points_args(a, cfg, vols, nullptr, packed, freq, phase, points, 0, cfg->B, n_per_image, nullptr)) return rc;
    a.rgb_sigma = rgb_sigma;
    if (hipError_t e = launch_forward(a, cfg, (hipStream_t)stream)) return hip_fail(e, "field kernel");
    return CNERF_OK;
}

int cnerf_composite(const cnerf_cfg* cfg, int64_t rays, int32_t n, const float* rgb_sigma, const float* z,
                    const float* eps, float* rgb, float* dist, float* weights, void* stream) {
    g_err[0] = 0;
    if (!cfg || rays < 1 || n < 1 || n > 256 || !rgb_sigma || !z) return fail(CNERF_EINVAL, "composite: bad argument (1 <= n <= 256)");
    CompositeArgs a{rgb_sigma, z, eps, rgb, dist, weights, (long long)rays, n, cfg->noise_std, cfg->flags};
    if (hipError_t e = launch_composite(a, (hipStream_t)stream)) return hip_fail(e, "composite");
    return CNERF_OK;
}

int cnerf_resample(int64_t rays, int32_t S, const float* z, const float* weights, const float* u, float* fine_z,
                   int32_t* inds, float* cdf, void* stream) {
    g_err[0] = 0;
    if (rays < 1 || S < 2 || S > 128 || !z || !weights || !u || !fine_z) return fail(CNERF_EINVAL, "resample: bad argument (2 <= S <= 128)");
    ResampleArgs a{z, weights, nullptr, nullptr, u, fine_z, inds, cdf, nullptr, (long long)rays, S, 0.0f, 0u, PhiloxKey{0u, 0u, 0u, 0u}};
    if (hipError_t e = launch_resample(a, (hipStream_t)stream)) return hip_fail(e, "resample");
    return CNERF_OK;
}

int cnerf_render_forward(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* freq,
                         const float* phase, const float* cam2world, const cnerf_rng* rng, float* pixels,
                         float* depth, const cnerf_aux* aux, void* workspace, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    if ((!vols && !no_volume(cfg)) || !packed || !cam2world || !pixels || !depth || !workspace) return fail(CNERF_EINVAL, "render_forward: NULL argument");
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "render_forward: FiLM layers need freq and phase");
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    rng = rng_or_none(rng);
    if (hier && !rng->u_fine && !cfg->philox) return fail(CNERF_EINVAL, "render_forward: hierarchical sampling needs rng.u_fine (or cfg.philox)");
    hipStream_t stream = (hipStream_t)stream_;

    const long long P = (long long)cfg->R * cfg->R, S = cfg->S;
    const long long npi = P * S;
    const ForwardLayout F = forward_layout(cfg);
    char* ws = (char*)workspace;
    float* c_rs = (float*)(ws + F.c_rs);
    float* f_rs = (float*)(ws + F.f_rs);
    float* c_z = (float*)(ws + F.c_z);
    float* f_z = (float*)(ws + F.f_z);
    if (aux) {   // write straight into the caller's buffers where given
        if (aux->coarse_rgb_sigma) c_rs = aux->coarse_rgb_sigma;
        if (aux->fine_rgb_sigma) f_rs = aux->fine_rgb_sigma;
        if (aux->coarse_z) c_z = aux->coarse_z;
        if (aux->fine_z) f_z = aux->fine_z;
    }

    FieldArgs fa;
    if (int rc = fill_field_args(fa, cfg, vols, nullptr, packed, freq, phase)) return rc;
    set_points(fa, cfg->B, npi);
    fa.cam2world = cam2world;
    // the exact fp32 precision: FiLM (plain sine: freq 1, phase 0) folded into one affine map per matrix and channel, prepared once
    // for both passes (per-point FiLM computes its frequencies per point: not foldable)
    if (cfg->precision == CNERF_PREC_FP32 && cfg->layer_kind[0] != CNERF_LAYER_PFILM && cfg->drop_p == 0.0f) {
        float* fold = (float*)(ws + F.fold);
        float* packed_img = (float*)(ws + F.packed_img);
        if (hipError_t e = launch_fold_film(fa, cfg->B, cfg->H, fold, stream)) return hip_fail(e, "fold_film");
        fa.fold = fold;
        fa.fold_images = cfg->B;
        // the scale goes into per-image copies of the layer weights (WFOLD, field_kernel.hip)
        if (hipError_t e = launch_scale_packed(fa, cfg->B, cfg->H, fold, F.layer_floats, packed_img, stream)) return hip_fail(e, "scale_packed");
        fa.packed_img = packed_img;
        fa.packed_img_stride = F.layer_floats;
    }
    // the fp16 precisions: the same folding on two-part fp16 weights -- per-image copies of the packed stream, the accumulators start
    // from (freq bias + phase) / 2 pi, the epilogue is one multiply, the range reduction and v_sin (field_h3.hip)
    if (cfg->precision != CNERF_PREC_FP32 && cfg->layer_kind[0] != CNERF_LAYER_PFILM) {
        void* img = ws + F.img16;
        float* fold16 = (float*)(ws + F.fold16);
        float* rowf = (float*)(ws + F.rowf);
        const long long img_elems = (long long)packed_layout(cfg).weight_floats * 2;      // fp16 elements of the packed weight stream
        if (hipError_t e = (cfg->precision == CNERF_PREC_FP16 ? launch_fold_h1 : launch_fold_h3)(fa, cfg->B, cfg->H, img, fold16, rowf, img_elems, stream))
            return hip_fail(e, "fold16");
        fa.packed_img = (const float*)img;
        fa.packed_img_stride = img_elems / 8;     // in f16x8 fragments
        fa.fold = fold16;
        fa.fold_images = cfg->B;
    }
    // 1. coarse pass
    fa.mode = FIELD_MODE_COARSE;
    fa.u_strat = rng->u_strat;
    fa.rgb_sigma = c_rs;
    fa.z_out = c_z;
    fa.points_out = aux ? aux->coarse_points : nullptr;
    auto mark = [&](int i) {
        if (aux && aux->field_events[i]) (void)hipEventRecord((hipEvent_t)aux->field_events[i], stream);
    };
    const bool keep = aux && aux->act16[0].h;
    if (keep) {
        if (cfg->precision != CNERF_PREC_FP16X3 && cfg->precision != CNERF_PREC_FP16)
            return fail(CNERF_EINVAL, "render_forward: act16 needs precision CNERF_PREC_FP16X3 or CNERF_PREC_FP16");
        if (!aux->act16[0].feat || !aux->act16[0].c || (hier && (!aux->act16[1].feat || !aux->act16[1].h || !aux->act16[1].c)))
            return fail(CNERF_EINVAL, "render_forward: act16 is incomplete");
        if (cfg->layer_kind[0] == CNERF_LAYER_PFILM) {
            if (cfg->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "render_forward: per-point FiLM keeps its activations in precision CNERF_PREC_FP16X3 only");
            if (!aux->act16[0].amax || (hier && !aux->act16[1].amax)) return fail(CNERF_EINVAL, "render_forward: act16.amax is NULL (per-point FiLM)");
        }
    }
    auto keep_pass = [&](int i) {
        fa.act_points = (long long)cfg->B * npi;
        fa.act_feat = keep ? (float*)aux->act16[i].feat : nullptr;
        fa.act_h = keep ? (float*)aux->act16[i].h : nullptr;
        fa.act_c = keep ? (float*)aux->act16[i].c : nullptr;
        fa.act_amax = keep ? (float*)aux->act16[i].amax : nullptr;
        fa.act_tb16 = keep ? 1 : 0;
    };
    keep_pass(0);
    set_dropout(fa, cfg, rng->drop_coarse, PHILOX_DROP_COARSE, npi);
    mark(0);
    if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, "field kernel (coarse)");
    mark(1);

    if (hier) {
        // 2. coarse weights -> inverse-CDF depths
        ResampleArgs ra{c_z, nullptr, c_rs, rng->eps_coarse, rng->u_fine, f_z, aux ? aux->inds : nullptr,
                        aux ? aux->cdf : nullptr, aux ? aux->coarse_weights : nullptr, (long long)cfg->B * P, (int)S,
                        cfg->noise_std, cfg->flags, philox_of(cfg)};
        if (hipError_t e = launch_resample(ra, stream)) return hip_fail(e, "resample");
        // 3. fine pass
        fa.mode = FIELD_MODE_FINE;
        fa.u_strat = nullptr;
        if (rng->fine_z) f_z = const_cast<float*>(rng->fine_z);   // teacher-forced depths (read only from here on)
        fa.fine_z = f_z;
        fa.rgb_sigma = f_rs;
        fa.z_out = nullptr;
        fa.points_out = aux ? aux->fine_points : nullptr;
        keep_pass(1);
        set_dropout(fa, cfg, rng->drop_fine, PHILOX_DROP_FINE, npi);
        mark(2);
        if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, "field kernel (fine)");
        mark(3);
    }
    // 4. merge + composite + epilogue
    MergeArgs ma{c_rs, c_z, hier ? f_rs : nullptr, hier ? f_z : nullptr, rng->eps_final, pixels, depth,
                 aux ? aux->sort_idx : nullptr, aux ? aux->final_weights : nullptr, (long long)cfg->B * P, (int)S,
                 make_geom(cfg), cfg->noise_std, cfg->flags, philox_of(cfg)};
    if (hipError_t e = launch_merge_composite(ma, stream)) return hip_fail(e, "merge_composite");
    return CNERF_OK;
}

int cnerf_backward_bytes(const cnerf_cfg* cfg, size_t* packed_t) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    const NetCounts nc = counts_of(cfg);
    const size_t NT = cfg->H / 32, tile = 4 * 64 * 4;
    size_t fl = NT * 2 * 64 + (size_t)(nc.n_mats - 1) * NT * NT * tile;     // head^T, the matrices after layer 0
    if (cfg->layer_kind[0] != CNERF_LAYER_PFILM && !no_volume(cfg))   // (per-point FiLM, no volume: the chain stops at layer 0's pre-activation)
        fl += (size_t)nc.n_in * NT * tile;                   // layer 0 transposed: one 32-row output tile per input tile
    if (packed_t) *packed_t = align256(fl * sizeof(float));
    return CNERF_OK;
}

int cnerf_pack_field_transposed(const cnerf_cfg* cfg, const cnerf_field_params* p, float* packed_t, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (!p || !packed_t) return fail(CNERF_EINVAL, "pack_field_transposed: NULL argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int H = cfg->H, NT = H / 32;
    const size_t tile = 4 * 64 * 4;
    float* dst = packed_t;
    if (!p->w_final) return fail(CNERF_EINVAL, "pack_field_transposed: head is NULL");
    if (hipError_t e = launch_pack_head_t(p->w_final, H, dst, stream)) return hip_fail(e, "pack_head_t");
    dst += (size_t)NT * 2 * 64;
    for (int l = cfg->L - 1; l >= 1; --l) {      // in the order the backward consumes them (a residual block: fc2 then fc1)
        if (!p->w[l]) return fail(CNERF_EINVAL, "pack_field_transposed: layer %d weight is NULL", l);
        if (cfg->layer_kind[l] == CNERF_LAYER_RES) {
            if (!p->w2[l]) return fail(CNERF_EINVAL, "pack_field_transposed: residual layer %d fc2 is NULL", l);
            if (hipError_t e = launch_pack_matrix_t(p->w2[l], H, H, NT, dst, stream)) return hip_fail(e, "pack_matrix_t");
            dst += (size_t)NT * NT * tile;
        }
        if (hipError_t e = launch_pack_matrix_t(p->w[l], H, H, NT, dst, stream)) return hip_fail(e, "pack_matrix_t");
        dst += (size_t)NT * NT * tile;
    }
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM || no_volume(cfg)) return CNERF_OK;      // head^T and W_l^T of layers L-1..1 only
    if (!p->w[0]) return fail(CNERF_EINVAL, "pack_field_transposed: layer 0 weight is NULL");
    const NetCounts nc = counts_of(cfg);
    if (hipError_t e = launch_pack_matrix_t(p->w[0], H, nc.k0, nc.n_in, dst, stream)) return hip_fail(e, "pack_matrix_t");
    return CNERF_OK;
}

int cnerf_merge_composite_backward(const cnerf_cfg* cfg, const float* coarse_rgb_sigma, const float* coarse_z,
                                   const float* fine_rgb_sigma, const float* fine_z, const float* eps_final,
                                   const float* grad_pixels, const float* grad_depth, float* grad_coarse,
                                   float* grad_fine, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    if (!coarse_rgb_sigma || !coarse_z || !grad_pixels || !grad_coarse) return fail(CNERF_EINVAL, "merge_composite_backward: NULL argument");
    if (hier && (!fine_rgb_sigma || !fine_z || !grad_fine)) return fail(CNERF_EINVAL, "merge_composite_backward: fine tensors missing");
    MergeBwdArgs a{coarse_rgb_sigma, coarse_z, hier ? fine_rgb_sigma : nullptr, hier ? fine_z : nullptr, eps_final,
                   grad_pixels, grad_depth, grad_coarse, hier ? grad_fine : nullptr,
                   (long long)cfg->B * cfg->R * cfg->R, cfg->S, make_geom(cfg), cfg->noise_std, cfg->flags, philox_of(cfg)};
    if (hipError_t e = launch_merge_composite_backward(a, (hipStream_t)stream)) return hip_fail(e, "merge_composite_backward");
    return CNERF_OK;
}

int cnerf_field_backward(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols,
                         const float* packed, const float* packed_t, const float* freq, const float* phase,
                         const float* cam2world, const float* u_strat, const float* fine_z,
                         const float* grad_rgb_sigma, const float* saved_rgb_sigma, float* act_feat, float* act_h,
                         float* act_c, float* act_g, float* act_go, const cnerf_grad_volumes* grad_vols, const uint8_t* drop_mask,
                         void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "field_backward: image range out of [0,B)");
    if (pass < 0 || pass > 2) return fail(CNERF_EINVAL, "field_backward: pass must be 0 (coarse), 1 (fine) or 2 (explicit points)");
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM && cfg->precision != CNERF_PREC_FP32)
        return fail(CNERF_EINVAL, "field_backward: the per-point FiLM family's fp32 chain needs a cfg (and packed weights) of precision fp32");
    const bool nv = no_volume(cfg);
    if ((!vols && !nv) || !packed || !packed_t || !cam2world || !grad_rgb_sigma || !saved_rgb_sigma || !act_feat || !act_h || !act_c ||
        !act_g || !act_go || (!grad_vols && !nv))
        return fail(CNERF_EINVAL, "field_backward: NULL argument");
    if (int rc = check_grad_vols(cfg, grad_vols, "field_backward")) return rc;
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "field_backward: the fine pass needs fine_z");
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "field_backward: FiLM layers need freq and phase");
    hipStream_t stream = (hipStream_t)stream_;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S;

    FieldArgs fa;
    if (int rc = pass_args(fa, cfg, pass, image0, n_images, vols, grad_vols, packed, freq, phase, cam2world, u_strat, fine_z)) return rc;
    set_dropout(fa, cfg, drop_mask, pass == 0 ? PHILOX_DROP_COARSE : pass == 1 ? PHILOX_DROP_FINE : PHILOX_DROP_POINTS, npi);
    return field_backward_run(fa, cfg, (long long)n_images * npi, packed_t, grad_rgb_sigma + (size_t)image0 * npi * 4,
                              saved_rgb_sigma + (size_t)image0 * npi * 4, act_feat, act_h, act_c, act_g, act_go, stream);
}

int cnerf_field_backward_points(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* packed, const float* packed_t, const float* freq,
                                const float* phase, const float* points, int64_t n_per_image, const float* grad_rgb_sigma,
                                const float* saved_rgb_sigma, float* act_feat, float* act_h, float* act_c, float* act_g, float* act_go,
                                const cnerf_grad_volumes* grad_vols, const uint8_t* drop_mask, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM && cfg->precision != CNERF_PREC_FP32)
        return fail(CNERF_EINVAL, "field_backward_points: the per-point FiLM family's fp32 chain needs a cfg (and packed weights) of precision fp32");
    const bool nv = no_volume(cfg);
    if ((!vols && !nv) || !packed || !packed_t || !points || n_per_image < 1 || !grad_rgb_sigma || !saved_rgb_sigma || !act_feat || !act_h || !act_c || !act_g ||
        !act_go || (!grad_vols && !nv))
        return fail(CNERF_EINVAL, "field_backward_points: NULL argument");
    if (int rc = check_grad_vols(cfg, grad_vols, "field_backward_points")) return rc;
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "field_backward_points: FiLM layers need freq and phase");
    FieldArgs fa;
    if (int rc = points_args(fa, cfg, vols, grad_vols, packed, freq, phase, points, 0, cfg->B, n_per_image, drop_mask)) return rc;
    return field_backward_run(fa, cfg, (long long)cfg->B * n_per_image, packed_t, grad_rgb_sigma, saved_rgb_sigma, act_feat, act_h, act_c, act_g,
                              act_go, (hipStream_t)stream);
}

int cnerf_scatter_patches(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const float* cam2world, const float* u_strat,
                          const float* fine_z, const float* gin, const cnerf_grad_volumes* grad_vols, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    if (no_volume(cfg)) return fail(CNERF_EINVAL, "scatter_patches: CNERF_F_NO_VOLUME networks have no volume to scatter into");
    if (pass != 0 && pass != 1) return fail(CNERF_EINVAL, "scatter_patches: pass must be 0 (coarse) or 1 (fine): explicit points are no pixel patches");
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "scatter_patches: image range out of [0,B)");
    if (!cam2world || !gin || !grad_vols) return fail(CNERF_EINVAL, "scatter_patches: NULL argument");
    if (int rc = check_grad_vols(cfg, grad_vols, "scatter_patches")) return rc;
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "scatter_patches: the fine pass needs fine_z");
    // the chunk's pass as cnerf_render_backward forms it for chunk16.  The scatter reads no volume, weight, freq or phase: the gradient
    // volumes stand in for the levels pass_args wants to see (it offsets their addresses and dereferences nothing)
    cnerf_volumes unread;
    memset(&unread, 0, sizeof(unread));
    for (int i = 0; i < n_levels_of(cfg); ++i) unread.level[i] = grad_vols->level[i];
    FieldArgs fa;
    if (int rc = pass_args(fa, cfg, pass, image0, n_images, &unread, grad_vols, nullptr, nullptr, nullptr, cam2world, u_strat, fine_z)) return rc;
    if (hipError_t e = launch_scatter_patch(fa, gin, (hipStream_t)stream)) return hip_fail(e, "scatter_patch");
    return CNERF_OK;
}

int cnerf_weight_grad16(int32_t n_images, int64_t tiles_per_image, int32_t n_rows, int32_t g_ct, int32_t x_ct, const void* G,
                        const void* X, float* dW, float* colsum, const float* inv_scale, void* stream) {
    g_err[0] = 0;
    if (!G || !X || !dW) return fail(CNERF_EINVAL, "weight_grad16: NULL argument");
    if (n_images < 1 || tiles_per_image < 1) return fail(CNERF_EINVAL, "weight_grad16: empty chunk");
    const int noc = (n_rows + 31) / 32;
    if (n_rows < 1 || (noc != 1 && noc != 2 && noc != 4 && noc != 8) || noc > g_ct || x_ct < 1 || x_ct > 8)
        return fail(CNERF_EINVAL, "weight_grad16: n_rows=%d (1..256, 1/2/4/8 channel tiles), g_ct=%d, x_ct=%d (1..8) unsupported", n_rows, g_ct, x_ct);
    if (hipError_t e = launch_weight_grad16(n_images, tiles_per_image, n_rows, g_ct, x_ct, G, X, dW, colsum, inv_scale, (hipStream_t)stream))
        return hip_fail(e, "weight_grad16");
    return CNERF_OK;
}

namespace {
// packed16 layout: [transposed units of matrices n_mats-1 .. 1, then layer 0 (output tiles padded to even)][head^T: NT fragments
// x 64 lanes][winv: n_mats + 1 floats, then ||W||_1: n_mats + 1 floats][max|W| scratch: n_mats + 1 uint32], each section
// 256-byte aligned
struct Chain16Layout {
    size_t units_bytes, head_off, winv_off, wmax_off, total;
    int n_mats, n_in, k0, ot0;
};
int chain16_layout(const cnerf_cfg* c, Chain16Layout& l) {
    if (c->layer_kind[0] == CNERF_LAYER_PFILM)         // (all layers or none, check_cfg)
        return fail(CNERF_ENOSYS, "half-precision backward: FiLM / plain-sine / residual layers only (layer 0 is per-point FiLM)");
    const size_t NT = c->H / 32, KCH = 2 * NT, frag = 64 * 16;
    const NetCounts nc = counts_of(c);
    l.n_mats = nc.n_mats;
    l.n_in = nc.n_in;
    l.k0 = nc.k0;
    l.ot0 = (nc.n_in + 1) / 2 * 2;
    l.units_bytes = ((size_t)(l.n_mats - 1) * NT + l.ot0) * KCH * frag;
    l.head_off = align256(l.units_bytes);
    l.winv_off = l.head_off + align256(NT * frag);
    l.wmax_off = l.winv_off + align256((size_t)2 * (l.n_mats + 1) * sizeof(float));
    l.total = l.wmax_off + align256((size_t)(l.n_mats + 1) * sizeof(uint32_t));
    return CNERF_OK;
}
}  // namespace

namespace {
// per-point FiLM family (chain_pw16.hip): [Y units][M units + Wm1^T][head^T: NT fragments x 64 lanes][winv: 2 L + 2][anorm: L + 1][max|W| scratch: 2 L + 2]
struct PwChainLayout {
    size_t m_off, head_off, winv_off, anorm_off, wmax_off, total;
};
PwChainLayout pw_chain_layout(const cnerf_cfg* c) {
    PwChainLayout l;
    const size_t NT = c->H / 32, L = c->L;
    l.m_off = align256(pw_chain_y_bytes(c->L, c->H));
    l.head_off = l.m_off + align256(pw_chain_m_bytes(c->L, c->H));
    l.winv_off = l.head_off + align256(NT * 1024);
    l.anorm_off = l.winv_off + align256((2 * L + 2) * sizeof(float));
    l.wmax_off = l.anorm_off + align256((L + 1) * sizeof(float));
    l.total = l.wmax_off + align256((2 * L + 2) * sizeof(uint32_t));
    return l;
}
}  // namespace

int cnerf_backward16_bytes(const cnerf_cfg* cfg, size_t* packed16) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM) {
        if (packed16) *packed16 = pw_chain_layout(cfg).total;
        return CNERF_OK;
    }
    Chain16Layout l;
    if (int rc = chain16_layout(cfg, l)) return rc;
    if (packed16) *packed16 = l.total;
    return CNERF_OK;
}

int cnerf_pack_field_chain16(const cnerf_cfg* cfg, const cnerf_field_params* p, void* packed16, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM) {
        if (!p || !packed16 || !p->w_final || !p->map_w1 || !p->map_w2) return fail(CNERF_EINVAL, "pack_field_chain16: NULL argument");
        for (int l = 1; l < cfg->L; ++l)
            if (!p->w[l]) return fail(CNERF_EINVAL, "pack_field_chain16: layer %d weight is NULL", l);
        if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "per-point FiLM: a single 32-channel feature volume is supported");
        const PwChainLayout l = pw_chain_layout(cfg);
        char* base = (char*)packed16;
        if (hipError_t e = launch_pack_pw_chain(p, cfg->L, cfg->H, base, base + l.m_off, base + l.head_off, (float*)(base + l.winv_off),
                                                (float*)(base + l.anorm_off), (uint32_t*)(base + l.wmax_off), (hipStream_t)stream_))
            return hip_fail(e, "pack_pw_chain");
        return CNERF_OK;
    }
    Chain16Layout l;
    if (int rc = chain16_layout(cfg, l)) return rc;
    if (!p || !packed16 || !p->w_final) return fail(CNERF_EINVAL, "pack_field_chain16: NULL argument");
    hipStream_t stream = (hipStream_t)stream_;
    const int H = cfg->H, NT = H / 32;
    const size_t KCH = 2 * NT, frag = 64 * 16;
    char* base = (char*)packed16;
    float* winv = (float*)(base + l.winv_off);
    uint32_t* wmax = (uint32_t*)(base + l.wmax_off);
    char* dst = base;
    const float* mats[2 * CNERF_MAX_LAYERS];         // the matrices in slab order (a residual block: fc1, fc2)
    int nm = 0;
    for (int i = 0; i < cfg->L; ++i) {
        if (!p->w[i]) return fail(CNERF_EINVAL, "pack_field_chain16: layer %d weight is NULL", i);
        mats[nm++] = p->w[i];
        if (cfg->layer_kind[i] == CNERF_LAYER_RES) {
            if (!p->w2[i]) return fail(CNERF_EINVAL, "pack_field_chain16: residual layer %d fc2 is NULL", i);
            mats[nm++] = p->w2[i];
        }
    }
    const int M = l.n_mats;
    for (int m = M - 1; m >= 1; --m) {               // consumption order of the chain
        if (hipError_t e = launch_pack_t16(mats[m], H, H, H, NT, dst, winv + m, wmax + m, stream)) return hip_fail(e, "pack_t16");
        dst += (size_t)NT * KCH * frag;
    }
    if (hipError_t e = launch_pack_t16(mats[0], H, l.k0, l.k0, l.ot0, dst, winv + 0, wmax + 0, stream)) return hip_fail(e, "pack_t16");
    if (hipError_t e = launch_pack_head_t16(p->w_final, H, base + l.head_off, winv + M, wmax + M, stream)) return hip_fail(e, "pack_head_t16");
    float* anorm = winv + M + 1;                       // ||W_m||_1 per matrix, then the head's (4 x H: max over channels of the 4-term sum)
    for (int m = 0; m < M; ++m)
        if (hipError_t e = launch_col_abs_sum_max(mats[m], H, m == 0 ? l.k0 : H, anorm + m, stream)) return hip_fail(e, "col_abs_sum_max");
    if (hipError_t e = launch_col_abs_sum_max(p->w_final, 4, H, anorm + M, stream)) return hip_fail(e, "col_abs_sum_max");
    return CNERF_OK;
}

namespace {
// Buffers of cnerf_pfilm_backward_finish (n = n_images * n_per_image rows), every piece 256-byte aligned:
//   packed_map = [Wm2 in pfilm_gm32_kernel's A-operand order: 2 L H * 256 floats][Wm1 in its chained product's: 256 * 32 floats]
//   workspace  = [g_mpre (n, 256)][d feat (n, 32): the rows the scatter reads when the caller passes no grad_feat]
struct PfilmFinishLayout {
    size_t packed_map, g_mpre, d_feat, total;
    int K2;
};
int pfilm_finish_layout(const cnerf_cfg* c, int n_images, long long npi, const char* who, PfilmFinishLayout& F) {
    if (int rc = check_cfg(c, false)) return rc;
    if (c->layer_kind[0] != CNERF_LAYER_PFILM) return fail(CNERF_EINVAL, "%s: per-point FiLM networks only (layer 0 is of kind %d)", who, c->layer_kind[0]);
    if (c->precision != CNERF_PREC_FP32)
        return fail(CNERF_EINVAL, "%s: a stage of the exact fp32 backward: cfg->precision must be CNERF_PREC_FP32 (the fp16 backward runs in cnerf_render_backward)", who);
    if (c->C != 32 || c->n_levels > 1) return fail(CNERF_EINVAL, "%s: single 32-channel volume only", who);
    if (n_images < 1 || npi < 1) return fail(CNERF_EINVAL, "%s: empty chunk (n_images=%d, n_per_image=%lld)", who, n_images, npi);
    const size_t n = (size_t)n_images * (size_t)npi;
    F.K2 = 2 * c->L * c->H;
    F.packed_map = align256(((size_t)F.K2 * 256 + 256 * 32) * sizeof(float));
    F.g_mpre = 0;
    F.d_feat = align256(n * 256 * sizeof(float));
    F.total = F.d_feat + align256(n * 32 * sizeof(float));
    return CNERF_OK;
}
bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
// The stage itself (pfilm_finish.hip) on validated arguments: cnerf_pfilm_backward_finish, and the chunk body of the one-call backward
int pfilm_finish_run(const cnerf_cfg* cfg, const PfilmFinishLayout& F, const void* packed_map, int n_images, long long n_per_image, const float* points,
                     const float* act_feat, const float* act_h, const float* act_g, const float* act_go, const cnerf_field_param_grads* G,
                     float* grad_fvol_cl, float* grad_feat, void* workspace, hipStream_t stream) {
    const int H = cfg->H, Lc = cfg->L;
    const long long n = (long long)n_images * n_per_image;
    const size_t slab = (size_t)n * H;
    const float* m = act_h + (size_t)Lc * slab;
    const float* Gm = act_g + (size_t)Lc * slab;
    float* g_mpre = (float*)((char*)workspace + F.g_mpre);
    float* d_feat = grad_feat ? grad_feat : (float*)((char*)workspace + F.d_feat);
    // the reductions over the chunk's rows run over all n of them at once and add to the caller's buffers themselves: no per-image partials
    if (G->w[0] || G->b[0])
        if (hipError_t e = launch_layer0_grad32(act_g, points, n, H, G->w[0], G->b[0], stream)) return hip_fail(e, "layer0_grad32");
    for (int l = 1; l < Lc; ++l)
        if (G->w[l] || G->b[l])
            if (hipError_t e = launch_weight_grad(1, n, H, H, act_g + (size_t)l * slab, act_h + (size_t)(l - 1) * slab, G->w[l], G->b[l], stream))
                return hip_fail(e, "weight_grad");
    if (G->w_final || G->b_final)
        if (hipError_t e = launch_head_grad32(act_go, act_h + (size_t)(Lc - 1) * slab, n, H, G->w_final, G->b_final, stream)) return hip_fail(e, "head_grad32");
    if (G->map_w2 || G->map_b2)
        if (hipError_t e = launch_weight_grad(1, n, F.K2, 256, Gm, m, G->map_w2, G->map_b2, stream)) return hip_fail(e, "weight_grad (Wm2)");
    if (!G->map_w1 && !G->map_b1 && !grad_fvol_cl && !grad_feat) return CNERF_OK;
    if (hipError_t e = launch_pfilm_gm32((const float*)packed_map, Gm, m, n, F.K2, g_mpre, d_feat, stream)) return hip_fail(e, "pfilm_gm32");
    if (G->map_w1 || G->map_b1)
        if (hipError_t e = launch_weight_grad(1, n, 256, 32, g_mpre, act_feat, G->map_w1, G->map_b1, stream)) return hip_fail(e, "weight_grad (Wm1)");
    if (grad_fvol_cl) {
        GatherArgs a{nullptr, points, nullptr, (long long)n_per_image, n_images, cfg->V, cfg->C, cfg->voxel_length / 2.0f};
        if (hipError_t e = launch_scatter(a, d_feat, grad_fvol_cl, stream)) return hip_fail(e, "scatter");
    }
    return CNERF_OK;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// the whole backward in one call
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// Workspace of cnerf_render_backward and cnerf_field_query_backward, carved in this order (every piece 256-byte aligned).  A chunk is
// cnt images of npi points each: n = cnt * npi (fp32 backward: row-major fp32 chunk matrices), T = cnt * tiles per image (fp16 backward:
// TB16 blocks).  N_out: rows of the whole call's d loss / d rgb_sigma the render derives from d(pixels, depth) (0 for a query).
struct BackwardLayout {
    size_t gc, gf;                                   // d loss / d rgb_sigma of the coarse / fine samples, whole call
    size_t a_feat, a_h, a_c, a_g, a_go;              // chunk buffers (a_feat / a_h / a_c absent when the forward kept its activations)
    size_t a_amax;                                   // per-point FiLM family, fp16: (L, T * 32) floats
    size_t a_gy;                                     // per-point FiLM family, fp16: L TB16 slabs of g_y
    size_t pts, fin, map;                            // per-point FiLM family, fp32: a ray pass's sample positions (n, 3); workspace and packed_map of
    PfilmFinishLayout F;                             // the mapping-network stage, laid out as F for a full chunk (a smaller last chunk keeps its offsets)
    size_t a_gin;                                    // fp16 chain: (feature input tiles, chunk points, 32) fp32 input-tile gradients for scatter_patch_kernel
    size_t gmax, scales;                             // fp16: sampled maxima (n_mats + 1 uint32), {S, 1/S} pairs (n_mats + 1)
    size_t dwarg, cs, dwh, csh;                      // per-image reductions of one matrix: (cnt, H, 32 * max tiles), (cnt, H), (cnt, 4, H), (cnt, 4)
    size_t total;
    int n_mats, n_in, k0;
};
// render: the chunks are ray passes (else the point ranges of a query, which carries its positions and has no pixel patches)
int chunk_layout(const cnerf_cfg* c, int bprec, int cnt, size_t npi, size_t N_out, bool hier, bool have_act16, bool render, const char* who,
                 BackwardLayout& L) {
    if (bprec != CNERF_PREC_FP32 && bprec != CNERF_PREC_FP16) return fail(CNERF_EINVAL, "%s: backward_precision must be CNERF_PREC_FP32 or CNERF_PREC_FP16", who);
    if (cnt < 1 || cnt > c->B) return fail(CNERF_EINVAL, "%s: images_per_chunk=%d out of [1,B]", who, cnt);
    const bool pfilm = c->layer_kind[0] == CNERF_LAYER_PFILM, half = bprec == CNERF_PREC_FP16;
    if (have_act16 && (!half || cnt != c->B)) return fail(CNERF_EINVAL, "%s: kept activations need the fp16 backward and images_per_chunk = B", who);
    if (half && c->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "%s: the fp16 backward re-runs the fp16x3 forward (cfg->precision)", who);
    if (pfilm && !half && c->precision != CNERF_PREC_FP32)
        return fail(CNERF_EINVAL, "%s: the per-point FiLM family's fp32 chain re-runs the fp32 kernel: cfg (and packed weights) of precision fp32", who);
    const NetCounts nc = counts_of(c);
    const size_t H = c->H, NT = H / 32, Lc = c->L, tpi = (npi + 31) / 32;
    const size_t n = (size_t)cnt * npi, T = (size_t)cnt * tpi;
    L = BackwardLayout{};
    L.n_in = pfilm ? 2 : nc.n_in;         // (per-point FiLM: the feature tile and the position's)
    L.k0 = nc.k0;
    L.n_mats = nc.n_mats;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    L.gc = take(N_out * 4 * sizeof(float));
    L.gf = take(hier ? N_out * 4 * sizeof(float) : 0);
    if (pfilm && !half) {       // the chunk matrices of cnerf_field_backward (include/cnerf.h), then what the mapping-network stage needs; it
                                // accumulates straight into the caller's gradients: no per-image reductions
        if (int rc = pfilm_finish_layout(c, cnt, (long long)npi, who, L.F)) return rc;
        L.a_feat = take(n * 32 * sizeof(float));
        L.a_h = take((Lc * n * H + n * 256) * sizeof(float));
        L.a_c = take(3 * Lc * n * H * sizeof(float));
        L.a_g = take(3 * Lc * n * H * sizeof(float));
        L.a_go = take(n * 4 * sizeof(float));
        L.pts = take(render ? n * 3 * sizeof(float) : 0);
        L.fin = take(L.F.total);
        L.map = take(L.F.packed_map);
        L.total = off;
        return CNERF_OK;
    }
    if (pfilm) {      // chain_pw16.hip: three stored derivatives and three gradient slabs per layer, m and g_mpre
        L.a_feat = take(have_act16 ? 0 : T * 2 * 2048);
        L.a_h = take(have_act16 ? 0 : (Lc * NT + 8) * T * 2048);
        L.a_c = take(have_act16 ? 0 : 3 * Lc * NT * T * 2048);
        L.a_amax = take(have_act16 ? 0 : Lc * T * 32 * sizeof(float));
        L.a_g = take((3 * Lc * NT + 8) * T * 2048);
        L.a_go = take(T * 2048);
        L.a_gy = take(Lc * NT * T * 2048);                          // two-kernel chain: g_y slabs
        L.gmax = take((5 * Lc + 2) * sizeof(uint32_t));             // 3 L + 2 sampled maxima, L of g_y, L of the stored derivatives
        L.scales = take((2 * (4 * Lc + 2) + 2 * Lc) * sizeof(float));   // {S, 1 / S} x (4 L + 2), then per layer {r, To}
    } else if (half) {
        L.a_feat = take(have_act16 ? 0 : T * L.n_in * 2048);
        L.a_h = take(have_act16 ? 0 : (size_t)L.n_mats * T * NT * 2048);
        L.a_c = take(have_act16 ? 0 : (size_t)L.n_mats * T * NT * 2048);
        L.a_g = take((size_t)L.n_mats * T * NT * 2048);
        L.a_go = take(T * 2048);
        L.a_gin = take(render && !no_volume(c) ? (size_t)L.n_in * n * 32 * sizeof(float) : 0);   // (no feature tile: no rows, no patch scatter)
    } else {
        L.a_feat = take(n * 32 * L.n_in * sizeof(float));
        L.a_h = take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_c = take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_g = take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_go = take(n * 4 * sizeof(float));
    }
    if (!pfilm) {
        L.gmax = take((size_t)(L.n_mats + 2) * sizeof(uint32_t));
        L.scales = take((size_t)2 * (L.n_mats + 1) * sizeof(float));
    }
    const size_t rows = pfilm ? 256 : H, kmax = pfilm ? 256 : 32 * (size_t)(L.n_in > (int)NT ? L.n_in : (int)NT);   // the largest reduced matrix
    L.dwarg = take((size_t)cnt * rows * kmax * sizeof(float));
    L.cs = take((size_t)cnt * rows * sizeof(float));
    L.dwh = take((size_t)cnt * 4 * H * sizeof(float));
    L.csh = take((size_t)cnt * 4 * sizeof(float));
    L.total = off;
    return CNERF_OK;
}
int backward_layout(const cnerf_cfg* c, int bprec, int cnt, bool have_act16, BackwardLayout& L) {
    const size_t npi = (size_t)c->R * c->R * c->S;
    return chunk_layout(c, bprec, cnt, npi, (size_t)c->B * npi, c->flags & CNERF_F_HIERARCHICAL, have_act16, true, "render_backward", L);
}

// Scales of a half-precision chunk before its dry run: {1, 1} for slots 0 .. head - 1, slot `head` {S, 1 / S} from the largest
// |d loss / d rgb_sigma| of the chunk (g_out, n floats), whose bit pattern lands in *gmax_head; the gmax_words maxima are zeroed first
int head_scales(const float* g_out, long long n, uint32_t* gmax, size_t gmax_words, uint32_t* gmax_head, float* scales, int head, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(gmax, 0, gmax_words * sizeof(uint32_t), stream)) return hip_fail(e, "memset");
    if (hipError_t e = launch_absmax_bits(g_out, n, gmax_head, stream)) return hip_fail(e, "absmax");
    if (hipError_t e = launch_pow2_scales(gmax_head, 1, scales + 2 * head, stream)) return hip_fail(e, "pow2_scales");
    for (int m = 0; m < head; ++m)
        if (hipError_t e = launch_fill(scales + 2 * m, 1.0f, 2, stream)) return hip_fail(e, "fill");
    return CNERF_OK;
}

// One weight reduction of a half-precision chunk (cnt images of tpi tiles): dw (cnt, n_rows, 32 x_ct) = G^T X and cs (cnt, n_rows) =
// column sums of G per image (G: TB16, g_ct channel tiles, stored times 1 / *inv_scale), then param_reduce adds columns [k0, k0 + k_real)
// to dW, db -- and, for a FiLM matrix, dfreq / dphase of the chunk's images
int reduce16(int cnt, long long tpi, int n_rows, int g_ct, int x_ct, const void* G, const void* X, const float* inv_scale, float* dw, float* cs,
             int k0, int k_real, const float* freq, int film_stride, const float* W, const float* b, float* dW, float* db, float* dfreq,
             float* dphase, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(dw, 0, (size_t)cnt * n_rows * 32 * x_ct * sizeof(float), stream)) return hip_fail(e, "memset");
    if (hipError_t e = hipMemsetAsync(cs, 0, (size_t)cnt * n_rows * sizeof(float), stream)) return hip_fail(e, "memset");
    if (hipError_t e = launch_weight_grad16(cnt, tpi, n_rows, g_ct, x_ct, G, X, dw, cs, inv_scale, stream)) return hip_fail(e, "weight_grad16");
    if (hipError_t e = launch_param_reduce(cnt, n_rows, 32 * x_ct, k_real, dw + k0, cs, freq, film_stride, W, b, dW, db, dfreq, dphase, stream))
        return hip_fail(e, "param_reduce");
    return CNERF_OK;
}

// Environment CNERF_SCATTER=chain: the half-precision chain adds the ray passes' feature-volume gradients with its own atomics instead of
// scatter_sorted_kernel (A/B runs and tests/test_gpu_parity.py::test_sorted_patch_scatter_matches_the_chain_scatter, which switches it
// within one process: read per call)
bool scatter_by_chain() {
    const char* s = getenv("CNERF_SCATTER");
    return s && !strcmp(s, "chain");
}

// ---- chunk bodies: one chunk of cnt images (from image b0 of the call) of npi points (tpi tiles) each.  The render runs them per ray
// pass and chunk of images, cnerf_field_query_backward per image and range of query points.
struct Chunk {
    int b0, cnt;
    long long npi, tpi;
};

// exact fp32: cnerf_field_backward's re-run and chain (fa: the chunk's pass with gradient volumes and dropout set), one weight_grad
// per matrix, the head
int chunk32(const cnerf_cfg* cfg, const MatrixSet& ms, const BackwardLayout& L, char* ws, const FieldArgs& fa, const Chunk& k,
            const float* packed_t, const float* g_out, const float* s_out, const float* freq, const cnerf_field_param_grads* G, float* grad_freq,
            float* grad_phase, hipStream_t stream) {
    const int H = cfg->H;
    const size_t n = (size_t)k.cnt * k.npi;
    float* a_feat = (float*)(ws + L.a_feat);
    float* a_h = (float*)(ws + L.a_h);
    float* a_c = (float*)(ws + L.a_c);
    float* a_g = (float*)(ws + L.a_g);
    float* a_go = (float*)(ws + L.a_go);
    float* dwarg = (float*)(ws + L.dwarg);
    float* cs = (float*)(ws + L.cs);
    if (int rc = field_backward_run(fa, cfg, (long long)n, packed_t, g_out, s_out, a_feat, a_h, a_c, a_g, a_go, stream)) return rc;
    for (int m = 0; m < L.n_mats; ++m) {
        const int K = m == 0 ? 32 * L.n_in : H;
        const float* X = m == 0 ? a_feat : a_h + (size_t)(m - 1) * n * H;
        if (hipError_t e = hipMemsetAsync(dwarg, 0, (size_t)k.cnt * H * K * sizeof(float), stream)) return hip_fail(e, "memset");
        if (hipError_t e = hipMemsetAsync(cs, 0, (size_t)k.cnt * H * sizeof(float), stream)) return hip_fail(e, "memset");
        if (int rc = cnerf_weight_grad(k.cnt, k.npi, H, K, a_g + (size_t)m * n * H, X, dwarg, cs, stream)) return rc;
        if (hipError_t e = launch_param_reduce(k.cnt, H, K, m == 0 ? L.k0 : H, dwarg, cs, ms.film(freq, m, k.b0), ms.film_stride, ms.W[m], ms.b[m], ms.dW[m],
                                               ms.db[m], ms.film(grad_freq, m, k.b0), ms.film(grad_phase, m, k.b0), stream))
            return hip_fail(e, "param_reduce");
    }
    if (G->w_final && G->b_final)
        if (hipError_t e = launch_head_grad32(a_go, a_h + (size_t)(L.n_mats - 1) * n * H, (long long)n, H, G->w_final, G->b_final, stream))
            return hip_fail(e, "head_grad32");
    return CNERF_OK;
}

// half precision, FiLM / plain-sine / residual networks (bwd16.hip): the storing re-run (fp16x3 kernel) unless the activations are given,
// the chain's dry run for the per-matrix scales, the chain, the patch scatter of the input-tile gradients (fc.gin set), one weight_grad16
// per matrix.  fc: the chunk's pass with gradient volumes.
int chunk16(const cnerf_cfg* cfg, const MatrixSet& ms, const BackwardLayout& L, char* ws, const void* packed_bwd, FieldArgs fc, const Chunk& k,
            const float* g_out, const float* s_out, void* a_feat, void* a_h, void* a_c, bool store, const float* freq,
            const cnerf_field_param_grads* G, float* grad_freq, float* grad_phase, uint32_t* saturated, hipStream_t stream) {
    const int H = cfg->H, NT = H / 32;
    const long long T = (long long)k.cnt * k.tpi;
    Chain16Layout cl;
    if (int rc = chain16_layout(cfg, cl)) return rc;
    const char* base16 = (const char*)packed_bwd;
    const float* winv = (const float*)(base16 + cl.winv_off);
    uint32_t* gmax = (uint32_t*)(ws + L.gmax);
    float* scales = (float*)(ws + L.scales);
    char* a_g = ws + L.a_g;
    char* a_go = ws + L.a_go;
    if (int rc = head_scales(g_out, (long long)k.cnt * k.npi * 4, gmax, L.n_mats + 2, gmax + L.n_mats + 1, scales, L.n_mats, stream)) return rc;
    const long long groups = (long long)k.cnt * ((k.tpi + 3) / 4);
    long long step = groups / 2048;                       // dry-run sampling: every 16th tile group once there are plenty
    step = step < 1 ? 1 : (step > 16 ? 16 : step);
    // the storing re-run and the dry run (fa) leave the gradient volumes alone; the chain (fc) adds to them
    FieldArgs fa = fc;
    for (float*& g : fa.lvl_grad) g = nullptr;
    fa.gin = nullptr;
    if (store)
        if (hipError_t e = launch_field_h3(storing_args(fa, (long long)k.cnt * k.npi, a_feat, a_h, a_c, nullptr, a_g), H, stream))
            return hip_fail(e, "field kernel (fp16 activation store)");
    fa.grad_out = fc.grad_out = g_out;
    fa.saved_out = fc.saved_out = s_out;
    if (hipError_t e = launch_chain16(fa, H, base16, base16 + cl.head_off, winv, scales, a_c, nullptr, nullptr, gmax, nullptr, cl.n_mats, 1, (int)step,
                                      stream))
        return hip_fail(e, "chain16 (dry run)");
    if (hipError_t e = launch_pow2_scales(gmax, L.n_mats, scales, stream)) return hip_fail(e, "pow2_scales");
    if (hipError_t e = launch_chain16(fc, H, base16, base16 + cl.head_off, winv, scales, a_c, a_g, a_go, nullptr, saturated, cl.n_mats, 0, 1, stream))
        return hip_fail(e, "chain16");
    if (fc.gin)
        if (hipError_t e = launch_scatter_patch(fc, fc.gin, stream)) return hip_fail(e, "scatter_patch");
    float* dwarg = (float*)(ws + L.dwarg);
    float* cs = (float*)(ws + L.cs);
    const size_t slab = (size_t)T * NT * 2048;             // bytes per matrix in a_h / a_g
    for (int m = 0; m < L.n_mats; ++m) {
        const int x_ct = m == 0 ? L.n_in : NT;
        const void* X = m == 0 ? a_feat : (const void*)((const char*)a_h + (size_t)(m - 1) * slab);
        if (int rc = reduce16(k.cnt, k.tpi, H, NT, x_ct, a_g + (size_t)m * slab, X, scales + 2 * m + 1, dwarg, cs, 0, m == 0 ? L.k0 : H,
                              ms.film(freq, m, k.b0), ms.film_stride, ms.W[m], ms.b[m], ms.dW[m], ms.db[m], ms.film(grad_freq, m, k.b0),
                              ms.film(grad_phase, m, k.b0), stream))
            return rc;
    }
    return reduce16(k.cnt, k.tpi, 4, 1, NT, a_go, (const char*)a_h + (size_t)(L.n_mats - 1) * slab, scales + 2 * L.n_mats + 1, (float*)(ws + L.dwh),
                    (float*)(ws + L.csh), 0, H, nullptr, 0, nullptr, nullptr, G->w_final, G->b_final, nullptr, nullptr, stream);
}

// half precision, per-point FiLM family: storing forward (field_pw16.hip) unless the activations are given, the two chain kernels with
// their dry runs (chain_pw16.hip), one weight_grad16 reduction per matrix: dW_l = g_pre_l^T y_{l-1}, dWm2 rows = (g_fr_l | g_ph_l)^T m,
// dWm1 = g_mpre^T feat, head.  fa: the chunk's pass with gradient volumes.
int chunk_pw16(const cnerf_cfg* cfg, const BackwardLayout& L, char* ws, const void* packed_bwd, FieldArgs fa, const Chunk& k, const float* g_out,
               const float* s_out, char* a_feat, char* a_h, char* a_c, float* a_amax, bool store, const cnerf_field_param_grads* G, uint32_t* saturated,
               hipStream_t stream) {
    const int H = cfg->H, NT = H / 32, Lc = cfg->L, n_slots = 3 * Lc + 2;
    const long long T = (long long)k.cnt * k.tpi;
    const PwChainLayout cl = pw_chain_layout(cfg);
    const char* base16 = (const char*)packed_bwd;
    uint32_t* gmax = (uint32_t*)(ws + L.gmax);
    float* scales = (float*)(ws + L.scales);
    char* a_g = ws + L.a_g;
    char* a_go = ws + L.a_go;
    float* dwarg = (float*)(ws + L.dwarg);
    float* cs = (float*)(ws + L.cs);
    if (store)
        if (hipError_t e = launch_field_pw3(storing_args(fa, (long long)k.cnt * k.npi, a_feat, a_h, a_c, a_amax, a_g), H, stream))
            return hip_fail(e, "field kernel (fp16 activation store)");
    fa.grad_out = g_out;
    fa.saved_out = s_out;
    if (int rc = head_scales(fa.grad_out, (long long)k.cnt * k.npi * 4, gmax, 5 * Lc + 2, gmax + n_slots - 1, scales, n_slots - 1, stream)) return rc;
    const size_t slabH = (size_t)T * NT * 2048;            // bytes per (tiles, NT, 32, 32) slab
    float* lay = scales + 2 * (4 * Lc + 2);
    PwChainBuffers cb{base16, base16 + cl.m_off, base16 + cl.head_off, (const float*)(base16 + cl.winv_off), (const float*)(base16 + cl.anorm_off),
                      scales, lay, a_c, a_amax, a_h + (size_t)Lc * slabH, ws + L.a_gy, a_g, a_go, gmax, nullptr};
    const long long groups = (long long)k.cnt * ((k.tpi + 3) / 4);
    long long step = groups / 1024;                       // dry-run sampling: at least 1024 tile groups (131 k points), every 32nd at most
    step = step < 1 ? 1 : (step > 32 ? 32 : step);
    // g_y through the layer matrices (dry run -> its scales), then the stored slabs and the mapping products (dry run -> g_mpre's scale)
    for (int m = 0; m < Lc; ++m)
        if (hipError_t e = launch_fill(scales + 2 * (3 * Lc + 2 + m), 1.0f, 2, stream)) return hip_fail(e, "fill");
    if (hipError_t e = launch_chain_pre(fa, H, cb, 1, (int)step, stream)) return hip_fail(e, "chain_pre (dry run)");
    if (hipError_t e = launch_pow2_scales(gmax + 3 * Lc + 2, Lc, scales + 2 * (3 * Lc + 2), stream)) return hip_fail(e, "pow2_scales");
    for (int m = 0; m < Lc; ++m)      // the largest stored derivative of each layer over the chunk's points
        if (hipError_t e = launch_absmax_bits(a_amax + (size_t)m * T * 32, T * 32, gmax + 4 * Lc + 2 + m, stream)) return hip_fail(e, "absmax");
    if (hipError_t e = launch_pw_split_scales(gmax + 4 * Lc + 2, Lc, scales, lay, stream)) return hip_fail(e, "split_scales");
    cb.sat = saturated;
    if (hipError_t e = launch_chain_pre(fa, H, cb, 0, 1, stream)) return hip_fail(e, "chain_pre");
    cb.sat = nullptr;
    if (hipError_t e = launch_pw_gm(fa, H, cb, 1, (int)step, stream)) return hip_fail(e, "pw_gm (dry run)");
    if (hipError_t e = launch_pow2_scales(gmax + 3 * Lc, 1, scales + 2 * (3 * Lc), stream)) return hip_fail(e, "pow2_scales");
    cb.sat = saturated;
    if (hipError_t e = launch_pw_gm(fa, H, cb, 0, 1, stream)) return hip_fail(e, "pw_gm");
    // one reduction per matrix: G (n_rows of slab `slot`) against X (x_ct channel tiles), k_real columns from column k0 on
    auto reduce = [&](const void* Gs, int g_ct, int n_rows, int slot, const void* X, int x_ct, int k0, int k_real, float* dW, float* db) {
        return reduce16(k.cnt, k.tpi, n_rows, g_ct, x_ct, Gs, X, scales + 2 * slot + 1, dwarg, cs, k0, k_real, nullptr, 0, nullptr, nullptr, dW, db,
                        nullptr, nullptr, stream);
    };
    const char* m16 = a_h + (size_t)Lc * slabH;
    const size_t LH = (size_t)Lc * H;
    for (int l = 0; l < Lc; ++l) {
        const char* g_pre = a_g + (size_t)(3 * l) * slabH;
        if (l == 0) {      // X = [feature | position]: the position's three columns
            if (int rc = reduce(g_pre, NT, H, 3 * l, a_feat, 2, 32, 3, G->w[0], G->b[0])) return rc;
        } else {
            if (int rc = reduce(g_pre, NT, H, 3 * l, a_h + (size_t)(l - 1) * slabH, NT, 0, H, G->w[l], G->b[l])) return rc;
        }
        if (int rc = reduce(g_pre + slabH, NT, H, 3 * l + 1, m16, 8, 0, 256, G->map_w2 + (size_t)l * H * 256, G->map_b2 + (size_t)l * H)) return rc;
        if (int rc = reduce(g_pre + 2 * slabH, NT, H, 3 * l + 2, m16, 8, 0, 256, G->map_w2 + (LH + (size_t)l * H) * 256, G->map_b2 + LH + (size_t)l * H))
            return rc;
    }
    if (int rc = reduce(a_g + (size_t)(3 * Lc) * slabH, 8, 256, 3 * Lc, a_feat, 2, 0, 32, G->map_w1, G->map_b1)) return rc;
    return reduce16(k.cnt, k.tpi, 4, 1, NT, a_go, a_h + (size_t)(Lc - 1) * slabH, scales + 2 * (n_slots - 1) + 1, (float*)(ws + L.dwh), (float*)(ws + L.csh),
                    0, H, nullptr, 0, nullptr, nullptr, G->w_final, G->b_final, nullptr, nullptr, stream);
}

// exact fp32, per-point FiLM family: cnerf_field_backward's re-run and chain (fa as for chunk32), then the mapping-network stage
// (pfilm_finish.hip), which adds every parameter gradient and the scatter of d feat to the caller's buffers and leaves the d feat rows
// at ws + L.fin + L.F.d_feat.  points: the chunk's positions (n, 3), or NULL for a ray pass -- its re-run writes them into the workspace.
int chunk_pw32(const cnerf_cfg* cfg, const BackwardLayout& L, char* ws, FieldArgs fa, const Chunk& k, const float* packed_t, const float* g_out,
               const float* s_out, const float* points, const cnerf_field_param_grads* G, hipStream_t stream) {
    float* a_feat = (float*)(ws + L.a_feat);
    float* a_h = (float*)(ws + L.a_h);
    float* a_g = (float*)(ws + L.a_g);
    float* a_go = (float*)(ws + L.a_go);
    if (!points) points = fa.points_out = (float*)(ws + L.pts);
    if (int rc = field_backward_run(fa, cfg, (long long)k.cnt * k.npi, packed_t, g_out, s_out, a_feat, a_h, (float*)(ws + L.a_c), a_g, a_go, stream)) return rc;
    return pfilm_finish_run(cfg, L.F, ws + L.map, k.cnt, k.npi, points, a_feat, a_h, a_g, a_go, G, fa.lvl_grad[0], nullptr, ws + L.fin, stream);
}

int pfilm_grads_complete(const cnerf_field_params* P, const cnerf_field_param_grads* G, int Lc, const char* who) {
    if (!P->map_w1 || !P->map_w2 || !P->w_final) return fail(CNERF_EINVAL, "%s: mapping network / head parameters are NULL", who);
    if (!G->map_w1 || !G->map_b1 || !G->map_w2 || !G->map_b2 || !G->w_final || !G->b_final)
        return fail(CNERF_EINVAL, "%s: per-point FiLM needs the mapping network's and the head's gradient buffers", who);
    for (int l = 0; l < Lc; ++l)
        if (!G->w[l] || !G->b[l]) return fail(CNERF_EINVAL, "%s: gradient buffers of layer %d are NULL", who, l);
    return CNERF_OK;
}
}  // namespace

int cnerf_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int32_t images_per_chunk, int32_t have_act16, size_t* bytes) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    BackwardLayout L;
    if (int rc = backward_layout(cfg, backward_precision, images_per_chunk, have_act16 != 0, L)) return rc;
    if (bytes) *bytes = L.total;
    return CNERF_OK;
}

int cnerf_render_backward(const cnerf_cfg* cfg, int32_t bprec, int32_t cnt_max, const cnerf_volumes* vols, const cnerf_field_params* P,
                          const float* packed, const void* packed_bwd, const float* freq, const float* phase, const float* cam2world,
                          const cnerf_rng* rng, const cnerf_saved* saved, const cnerf_aux* kept, const float* grad_pixels,
                          const float* grad_depth, const cnerf_field_param_grads* G, float* grad_freq, float* grad_phase,
                          const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* workspace, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    const bool have_act16 = kept && kept->act16[0].h;
    BackwardLayout L;
    if (int rc = backward_layout(cfg, bprec, cnt_max, have_act16, L)) return rc;
    const bool nv = no_volume(cfg);
    if ((!vols && !nv) || !P || !packed || !packed_bwd || !cam2world || !saved || !grad_pixels || !G || (!grad_vols && !nv) || !workspace)
        return fail(CNERF_EINVAL, "render_backward: NULL argument");
    if (int rc = check_grad_vols(cfg, grad_vols, "render_backward")) return rc;
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    if (!saved->coarse_rgb_sigma || !saved->coarse_z || (hier && (!saved->fine_rgb_sigma || !saved->fine_z)))
        return fail(CNERF_EINVAL, "render_backward: saved rgb_sigma / z of the forward are incomplete");
    if (counts_of(cfg).n_film && (!freq || !phase || !grad_freq || !grad_phase))
        return fail(CNERF_EINVAL, "render_backward: FiLM layers need freq, phase and their gradient buffers");
    const bool pfilm = cfg->layer_kind[0] == CNERF_LAYER_PFILM, half = bprec == CNERF_PREC_FP16;
    MatrixSet ms;
    if (pfilm) {
        if (int rc = pfilm_grads_complete(P, G, cfg->L, "render_backward")) return rc;
        if (!half && misaligned16(workspace)) return fail(CNERF_EINVAL, "render_backward: workspace must be 16-byte aligned");
    } else if (int rc = matrix_set(cfg, P, G, "render_backward", ms)) return rc;
    rng = rng_or_none(rng);
    hipStream_t stream = (hipStream_t)stream_;
    const int B = cfg->B;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S, tpi = (npi + 31) / 32;
    char* ws = (char*)workspace;
    float* gc = (float*)(ws + L.gc);
    float* gf = hier ? (float*)(ws + L.gf) : nullptr;

    // 1. d(pixels, depth) -> d(rgb_sigma) of every coarse / fine sample
    if (int rc = cnerf_merge_composite_backward(cfg, saved->coarse_rgb_sigma, saved->coarse_z, saved->fine_rgb_sigma, saved->fine_z,
                                                cfg->noise_std != 0.0f ? rng->eps_final : nullptr, grad_pixels, grad_depth, gc, gf, stream_))
        return rc;

    if (pfilm && !half)      // the mapping-network stage's operands, packed once per call
        if (hipError_t e = launch_pack_pfilm_map(P->map_w1, P->map_w2, L.F.K2, (float*)(ws + L.map), stream)) return hip_fail(e, "pack_pfilm_map");
    // half precision: only channels 0..3 of a row of the head gradient are ever written: the rest must read as zero
    if (half)
        if (hipError_t e = hipMemsetAsync(ws + L.a_go, 0, (size_t)cnt_max * tpi * 2048, stream)) return hip_fail(e, "memset");
    // FiLM / plain-sine / residual networks in half precision: the chain stores its input-tile gradients (fp32, 128 B per point) and
    // scatter_sorted_kernel adds them to the volume pre-reduced per pixel patch (scatter_patch.hip), or the chain adds them itself
    // (CNERF_SCATTER=chain; a network without a volume has nothing to scatter)
    float* gin = half && !pfilm && !scatter_by_chain() && !nv ? (float*)(ws + L.a_gin) : nullptr;

    // 2. per ray pass and chunk of images: the chunk body of the layer family and backward precision
    for (int pass = 0; pass < (hier ? 2 : 1); ++pass) {
        for (int b0 = 0; b0 < B; b0 += cnt_max) {
            const Chunk k{b0, b0 + cnt_max <= B ? cnt_max : B - b0, npi, tpi};
            const float* g_out = (pass ? gf : gc) + (size_t)b0 * npi * 4;
            const float* s_out = (pass ? saved->fine_rgb_sigma : saved->coarse_rgb_sigma) + (size_t)b0 * npi * 4;
            FieldArgs fa;       // the chunk's pass with the gradient volumes; dropout is the fp32 kernels' alone
            if (int rc = pass_args(fa, cfg, pass, b0, k.cnt, vols, grad_vols, packed, freq, phase, cam2world, rng->u_strat, saved->fine_z)) return rc;
            if (!half) set_dropout(fa, cfg, pass ? rng->drop_fine : rng->drop_coarse, pass ? PHILOX_DROP_FINE : PHILOX_DROP_COARSE, npi);
            fa.gin = gin;
            // the pass's activations (fp16 backward): kept by the forward (all images), or re-computed into the workspace
            char* a_feat = have_act16 ? (char*)kept->act16[pass].feat : ws + L.a_feat;
            char* a_h = have_act16 ? (char*)kept->act16[pass].h : ws + L.a_h;
            char* a_c = have_act16 ? (char*)kept->act16[pass].c : ws + L.a_c;
            float* a_amax = have_act16 ? (float*)kept->act16[pass].amax : (float*)(ws + L.a_amax);
            if (have_act16 && (!a_feat || !a_h || !a_c || (pfilm && !a_amax))) return fail(CNERF_EINVAL, "render_backward: act16 of pass %d is incomplete", pass);
            if (int rc = pfilm && half ? chunk_pw16(cfg, L, ws, packed_bwd, fa, k, g_out, s_out, a_feat, a_h, a_c, a_amax, !have_act16, G, saturated, stream)
                       : pfilm         ? chunk_pw32(cfg, L, ws, fa, k, (const float*)packed_bwd, g_out, s_out, nullptr, G, stream)
                       : half          ? chunk16(cfg, ms, L, ws, packed_bwd, fa, k, g_out, s_out, a_feat, a_h, a_c, !have_act16, freq, G, grad_freq, grad_phase,
                                                 saturated, stream)
                                       : chunk32(cfg, ms, L, ws, fa, k, (const float*)packed_bwd, g_out, s_out, freq, G, grad_freq, grad_phase, stream))
                return rc;
        }
    }
    return CNERF_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// gradients of a field query (autograd twin of cnerf_field_forward)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// Behind the chunk buffers of chunk_layout(cnt = 1, npi = points_per_chunk): the input-gradient rows of the position gradient
// (points_per_chunk, 256) fp32 -- feature columns, then the xyz columns -- and, with dropout, the keep bytes of the chunk
// (n_drop, points_per_chunk, H).
struct QueryLayout {
    BackwardLayout L;
    size_t rows, mask, total;
};
int query_layout(const cnerf_cfg* c, int bprec, long long ppc, QueryLayout& Q) {
    if (ppc < 1) return fail(CNERF_EINVAL, "field_query_backward: points_per_chunk=%lld must be >= 1", ppc);
    if (int rc = chunk_layout(c, bprec, 1, (size_t)ppc, 0, false, false, false, "field_query_backward", Q.L)) return rc;
    Q.rows = Q.L.total;
    Q.mask = Q.rows + align256((size_t)ppc * 256 * sizeof(float));
    Q.total = Q.mask + align256(c->drop_p > 0.0f ? (size_t)counts_of(c).n_drop * ppc * c->H : 0);
    return CNERF_OK;
}
}  // namespace

int cnerf_field_query_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int64_t points_per_chunk, size_t* bytes) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    QueryLayout Q;
    if (int rc = query_layout(cfg, backward_precision, (long long)points_per_chunk, Q)) return rc;
    if (bytes) *bytes = Q.total;
    return CNERF_OK;
}

namespace {
// cnerf_field_query_backward.  check_only: every refusal and no launch -- cnerf_render_rays_backward checks both of its field passes this
// way before its first kernel (points, saved_rgb_sigma, grad_rgb_sigma, workspace: any non-NULL placeholders then)
int query_backward(bool check_only, const cnerf_cfg* cfg, int32_t bprec, int64_t points_per_chunk, const cnerf_volumes* vols, const cnerf_field_params* P,
                   const float* packed, const void* packed_bwd, const float* freq, const float* phase, const float* points, int64_t n_per_image,
                   const float* saved_rgb_sigma, const float* grad_rgb_sigma, const cnerf_field_param_grads* G, float* grad_freq, float* grad_phase,
                   const cnerf_grad_volumes* grad_vols, float* grad_points, uint32_t* saturated, void* workspace, void* stream_) {
    if (int rc = check_cfg(cfg, false)) return rc;
    QueryLayout Q;
    if (int rc = query_layout(cfg, bprec, (long long)points_per_chunk, Q)) return rc;
    const BackwardLayout& L = Q.L;
    const bool nv = no_volume(cfg);
    if ((!vols && !nv) || !P || !packed || !packed_bwd || !points || !saved_rgb_sigma || !grad_rgb_sigma || !G || (!grad_vols && !nv) || !workspace || n_per_image < 1)
        return fail(CNERF_EINVAL, "field_query_backward: NULL argument or no points");
    if (int rc = check_grad_vols(cfg, grad_vols, "field_query_backward")) return rc;
    if (counts_of(cfg).n_film && (!freq || !phase || !grad_freq || !grad_phase))
        return fail(CNERF_EINVAL, "field_query_backward: FiLM layers need freq, phase and their gradient buffers");
    const bool pfilm = cfg->layer_kind[0] == CNERF_LAYER_PFILM;
    if (pfilm) {
        if (int rc = pfilm_grads_complete(P, G, cfg->L, "field_query_backward")) return rc;
        if (grad_points && !P->w[0]) return fail(CNERF_EINVAL, "field_query_backward: layer 0 weight is NULL");
        if (bprec == CNERF_PREC_FP32 && misaligned16(workspace)) return fail(CNERF_EINVAL, "field_query_backward: workspace must be 16-byte aligned");
    }
    MatrixSet ms;
    if (!pfilm)
        if (int rc = matrix_set(cfg, P, G, "field_query_backward", ms)) return rc;
    if (check_only) return CNERF_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const bool half = bprec == CNERF_PREC_FP16;
    const int B = cfg->B, H = cfg->H, NT = H / 32;
    const long long n = (long long)n_per_image, ppc = points_per_chunk < n ? (long long)points_per_chunk : n;
    char* ws = (char*)workspace;
    float* rows = (float*)(ws + Q.rows);
    uint8_t* mask = (uint8_t*)(ws + Q.mask);
    // only channels 0..3 of a row of the half-precision head gradient are ever written: the rest must read as zero
    if (half)
        if (hipError_t e = hipMemsetAsync(ws + L.a_go, 0, (size_t)((ppc + 31) / 32) * 2048, stream)) return hip_fail(e, "memset");
    if (pfilm && !half)      // the mapping-network stage's operands, packed once per call
        if (hipError_t e = launch_pack_pfilm_map(P->map_w1, P->map_w2, L.F.K2, (float*)(ws + L.map), stream)) return hip_fail(e, "pack_pfilm_map");
    for (int b = 0; b < B; ++b) {
        for (long long p0 = 0; p0 < n; p0 += ppc) {
            const long long np = p0 + ppc <= n ? ppc : n - p0;
            const Chunk k{b, 1, np, (np + 31) / 32};
            const size_t row0 = (size_t)b * n + p0;
            const float* pts = points + row0 * 3;
            const float* g_out = grad_rgb_sigma + row0 * 4;
            const float* s_out = saved_rgb_sigma + row0 * 4;
            // the chunk's field pass: image b, points [p0, p0 + np), with the gradient volumes; points are no pixel patches: the half-
            // precision chain adds its input-tile gradients with its own atomics (fa.gin stays NULL)
            FieldArgs fa;
            if (int rc = points_args(fa, cfg, vols, grad_vols, packed, freq, phase, pts, b, 1, np, nullptr)) return rc;
            if (cfg->drop_p > 0.0f) {
                // the forward's decisions of these points (Philox stream PHILOX_DROP_POINTS at their index in the whole call), as keep bytes
                // with chunk-local rows: the kernels index them by (image0 + b) * n_per_image + point = the point's row in the chunk
                if (hipError_t e = launch_drop_keep(fa.philox, PHILOX_DROP_POINTS, fa.drop_thresh, fa.n_drop, H, (unsigned long long)row0, np, mask, stream))
                    return hip_fail(e, "drop_keep");
                fa.drop_mask = mask;
                fa.drop_points = np;
                fa.image0 = 0;
            }
            if (int rc = pfilm && half ? chunk_pw16(cfg, L, ws, packed_bwd, fa, k, g_out, s_out, ws + L.a_feat, ws + L.a_h, ws + L.a_c, (float*)(ws + L.a_amax),
                                                    true, G, saturated, stream)
                       : pfilm         ? chunk_pw32(cfg, L, ws, fa, k, (const float*)packed_bwd, g_out, s_out, pts, G, stream)
                       : half          ? chunk16(cfg, ms, L, ws, packed_bwd, fa, k, g_out, s_out, ws + L.a_feat, ws + L.a_h, ws + L.a_c, true, freq, G,
                                                 grad_freq, grad_phase, saturated, stream)
                                       : chunk32(cfg, ms, L, ws, fa, k, (const float*)packed_bwd, g_out, s_out, freq, G, grad_freq, grad_phase, stream))
                return rc;
            if (!grad_points) continue;
            // position gradient: layer 0's input gradient [feature | xyz] = (g_0 (.) freq_0) W_0 from the chunk's layer-0 gradient slab, then
            // its lookup term plus the xyz columns.  Per-point FiLM: layer 0 reads the position alone (g_pre_0 W_0), the feature columns
            // are g_mpre Wm1 -- fp16: slot 3 L, 8 channel tiles; fp32: the d feat rows the mapping-network stage left
            const float* scales = (const float*)(ws + L.scales);
            const float* gfeat = rows;
            int ldf = 256;
            InputGradArgs ig{};
            ig.out = rows;
            ig.ldo = 256;
            ig.n = np;
            if (pfilm && half) {
                ig.g16 = ws + L.a_g + (size_t)(3 * cfg->L) * k.tpi * NT * 2048;
                ig.g_ct = 8;
                ig.inv_scale = scales + 2 * (3 * cfg->L) + 1;
                ig.W = P->map_w1;
                ig.K = 256;
                ig.k_in = cfg->C;
                if (hipError_t e = launch_input_grad(ig, stream)) return hip_fail(e, "input_grad");
            } else if (pfilm) {
                gfeat = (const float*)(ws + L.fin + L.F.d_feat);
                ldf = 32;
            }
            if (half) {
                ig.g16 = ws + L.a_g;
                ig.g_ct = NT;
                ig.inv_scale = scales + 1;
            } else {
                ig.g32 = (const float*)(ws + L.a_g);
                ig.ldg = H;
            }
            ig.f = pfilm ? nullptr : ms.film(freq, 0, b);
            ig.W = pfilm ? P->w[0] : ms.W[0];
            ig.K = H;
            ig.k_in = L.k0;
            ig.out = pfilm ? rows + cfg->C : rows;
            if (hipError_t e = launch_input_grad(ig, stream)) return hip_fail(e, "input_grad");
            PointsGradArgs pg = points_grad_args(cfg, vols, b, pts, grad_points + row0 * 3, np);
            pg.gfeat = gfeat;
            pg.ldf = ldf;
            pg.gxyz = (pfilm || (cfg->flags & (CNERF_F_INPUT_XYZ | CNERF_F_NO_VOLUME))) ? rows + cfg->C : nullptr;   // (no volume: C = 0, the xyz term alone)
            pg.ldx = 256;
            if (hipError_t e = launch_points_lookup_grad(pg, stream)) return hip_fail(e, "points_lookup_grad");
        }
    }
    return CNERF_OK;
}
}  // namespace

int cnerf_field_query_backward(const cnerf_cfg* cfg, int32_t bprec, int64_t points_per_chunk, const cnerf_volumes* vols, const cnerf_field_params* P,
                               const float* packed, const void* packed_bwd, const float* freq, const float* phase, const float* points,
                               int64_t n_per_image, const float* saved_rgb_sigma, const float* grad_rgb_sigma, const cnerf_field_param_grads* G,
                               float* grad_freq, float* grad_phase, const cnerf_grad_volumes* grad_vols, float* grad_points, uint32_t* saturated,
                               void* workspace, void* stream) {
    g_err[0] = 0;
    return query_backward(false, cfg, bprec, points_per_chunk, vols, P, packed, packed_bwd, freq, phase, points, n_per_image, saved_rgb_sigma,
                          grad_rgb_sigma, G, grad_freq, grad_phase, grad_vols, grad_points, saturated, workspace, stream);
}

int cnerf_feature_points_grad(const cnerf_cfg* cfg, const cnerf_volumes* vols, const float* points, int64_t n_per_image, const float* grad_feat,
                              float* grad_points, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (no_volume(cfg)) return fail(CNERF_EINVAL, "feature_points_grad: CNERF_F_NO_VOLUME networks look nothing up");
    if (!vols || !points || !grad_feat || !grad_points || n_per_image < 1) return fail(CNERF_EINVAL, "feature_points_grad: bad argument");
    for (int i = 0; i < n_levels_of(cfg); ++i)
        if (!vols->level[i]) return fail(CNERF_EINVAL, "feature_points_grad: volume level %d is NULL", i);
    for (int b = 0; b < cfg->B; ++b) {
        const size_t row0 = (size_t)b * n_per_image;
        PointsGradArgs pg = points_grad_args(cfg, vols, b, points + row0 * 3, grad_points + row0 * 3, n_per_image);
        pg.gfeat = grad_feat + row0 * cfg->C;
        pg.ldf = cfg->C;
        if (hipError_t e = launch_points_lookup_grad(pg, (hipStream_t)stream)) return hip_fail(e, "points_lookup_grad");
    }
    return CNERF_OK;
}

int cnerf_dropout_keep(const cnerf_cfg* cfg, uint32_t stream_id, int64_t point0, int64_t n_points, uint8_t* mask, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, false)) return rc;
    if (!mask || point0 < 0 || n_points < 1 || stream_id < PHILOX_DROP_COARSE || stream_id > PHILOX_DROP_POINTS || !(cfg->drop_p > 0.0f))
        return fail(CNERF_EINVAL, "dropout_keep: bad argument (drop_p > 0, stream 4..6)");
    const NetCounts nc = counts_of(cfg);
    if (hipError_t e = launch_drop_keep(philox_of(cfg), stream_id, nc.drop_thresh, nc.n_drop, cfg->H, (unsigned long long)point0, (long long)n_points, mask,
                                        (hipStream_t)stream))
        return hip_fail(e, "drop_keep");
    return CNERF_OK;
}

int cnerf_pfilm_finish_bytes(const cnerf_cfg* cfg, int32_t n_images, int64_t n_per_image, size_t* packed_map, size_t* workspace) {
    g_err[0] = 0;
    PfilmFinishLayout F;
    if (int rc = pfilm_finish_layout(cfg, n_images, (long long)n_per_image, "pfilm_finish_bytes", F)) return rc;
    if (packed_map) *packed_map = F.packed_map;
    if (workspace) *workspace = F.total;
    return CNERF_OK;
}

int cnerf_pack_pfilm_map_transposed(const cnerf_cfg* cfg, const cnerf_field_params* p, void* packed_map, void* stream) {
    g_err[0] = 0;
    PfilmFinishLayout F;
    if (int rc = pfilm_finish_layout(cfg, 1, 1, "pack_pfilm_map_transposed", F)) return rc;
    if (!p || !packed_map || !p->map_w1 || !p->map_w2) return fail(CNERF_EINVAL, "pack_pfilm_map_transposed: NULL argument (map_w1, map_w2, packed_map)");
    if (misaligned16(packed_map)) return fail(CNERF_EINVAL, "pack_pfilm_map_transposed: packed_map must be 16-byte aligned");
    if (hipError_t e = launch_pack_pfilm_map(p->map_w1, p->map_w2, F.K2, (float*)packed_map, (hipStream_t)stream)) return hip_fail(e, "pack_pfilm_map");
    return CNERF_OK;
}

int cnerf_pfilm_backward_finish(const cnerf_cfg* cfg, const cnerf_field_params* params, const void* packed_map, int32_t n_images, int64_t n_per_image,
                                const float* points, const float* act_feat, const float* act_h, const float* act_g, const float* act_go,
                                const cnerf_field_param_grads* G, float* grad_fvol_cl, float* grad_feat, void* workspace, void* stream_) {
    g_err[0] = 0;
    (void)params;      // the stage reads both mapping matrices from packed_map
    PfilmFinishLayout F;
    if (int rc = pfilm_finish_layout(cfg, n_images, (long long)n_per_image, "pfilm_backward_finish", F)) return rc;
    if (!packed_map || !points || !act_feat || !act_h || !act_g || !act_go || !G || !workspace)
        return fail(CNERF_EINVAL, "pfilm_backward_finish: NULL argument (packed_map, points, act_feat, act_h, act_g, act_go, grads, workspace)");
    if (misaligned16(packed_map) || misaligned16(act_feat) || misaligned16(act_h) || misaligned16(act_g) || misaligned16(act_go) || misaligned16(grad_feat) ||
        misaligned16(workspace))
        return fail(CNERF_EINVAL, "pfilm_backward_finish: packed_map, act_*, grad_feat and workspace must be 16-byte aligned");
    return pfilm_finish_run(cfg, F, packed_map, n_images, (long long)n_per_image, points, act_feat, act_h, act_g, act_go, G, grad_fvol_cl, grad_feat, workspace,
                            (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------------------------------------------------
// ray batches: the render on caller-given rays (B, P) instead of the R x R pinhole grid
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_rays_cfg(const cnerf_cfg* c, long long P, const char* who) {
    if (int rc = check_cfg(c, false)) return rc;
    if (c->S < 2 || c->S > 128) return fail(CNERF_EINVAL, "%s: S=%d out of range [2,128]", who, c->S);
    if (P < 1) return fail(CNERF_EINVAL, "%s: rays_per_image=%lld must be >= 1", who, P);
    if (c->drop_p > 0.0f) return fail(CNERF_EINVAL, "%s: dropout (drop_p > 0) is not implemented for ray batches (cnerf_render_forward has it)", who);
    return CNERF_OK;
}
int check_rays(const cnerf_rays* r, const char* who) {
    if (!r) return fail(CNERF_EINVAL, "%s: rays is NULL", who);
    if (!r->origins || !r->dirs) return fail(CNERF_EINVAL, "%s: rays.origins / rays.dirs is NULL", who);
    return CNERF_OK;
}
// per-ray sampling interval of the coarse pass: both arrays, or neither (a NULL struct or NULL members: the scalars of cfg)
int ray_bounds_of(const cnerf_ray_bounds* b, const char* who, const float*& near, const float*& far) {
    near = b ? b->near : nullptr;
    far = b ? b->far : nullptr;
    if (!near != !far) return fail(CNERF_EINVAL, "%s: bounds.near and bounds.far must both be given, or both be NULL", who);
    return CNERF_OK;
}
// Workspace of cnerf_render_rays_forward (every piece 256-byte aligned): the coarse and fine rgb_sigma (N, 4) and z (N), the sample
// positions of the pass in flight (N, 3); N = B P S
struct RaysForwardLayout {
    size_t c_rs, f_rs, c_z, f_z, pts, total;
};
RaysForwardLayout rays_forward_layout(const cnerf_cfg* c, long long P) {
    const size_t N = (size_t)c->B * (size_t)P * c->S;
    RaysForwardLayout F{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    F.c_rs = take(N * 4 * sizeof(float));
    F.f_rs = take(N * 4 * sizeof(float));
    F.c_z = take(N * sizeof(float));
    F.f_z = take(N * sizeof(float));
    F.pts = take(N * 3 * sizeof(float));
    F.total = off;
    return F;
}
// Workspace of cnerf_render_rays_backward: d loss / d rgb_sigma of the coarse and fine samples (N, 4), the positions of the pass in flight
// and their gradients (N, 3 each), then the workspace of a field query of P S points per image
struct RaysBackwardLayout {
    size_t gc, gf, pts, gpts, query, total;
};
int rays_backward_layout(const cnerf_cfg* c, int bprec, long long P, long long ppc, RaysBackwardLayout& R) {
    QueryLayout Q;
    if (int rc = query_layout(c, bprec, ppc, Q)) return rc;
    const size_t N = (size_t)c->B * (size_t)P * c->S;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    R.gc = take(N * 4 * sizeof(float));
    R.gf = take((c->flags & CNERF_F_HIERARCHICAL) ? N * 4 * sizeof(float) : 0);
    R.pts = take(N * 3 * sizeof(float));
    R.gpts = take(N * 3 * sizeof(float));
    R.query = take(Q.total);
    R.total = off;
    return CNERF_OK;
}
}  // namespace

int cnerf_render_rays_workspace_bytes(const cnerf_cfg* cfg, int64_t rays_per_image, size_t* fwd_ws) {
    g_err[0] = 0;
    if (int rc = check_rays_cfg(cfg, (long long)rays_per_image, "render_rays_workspace_bytes")) return rc;
    if (fwd_ws) *fwd_ws = rays_forward_layout(cfg, (long long)rays_per_image).total;
    return CNERF_OK;
}

// cnerf_render_rays_forward and cnerf_render_rays_bounded_forward (bounds == NULL: the scalars of cfg)
static int render_rays_forward_impl(const char* who, const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_ray_bounds* bounds,
                                    const cnerf_volumes* vols, const float* packed, const float* freq, const float* phase, const cnerf_rng* rng,
                                    float* pixels, float* dist, const cnerf_aux* aux, void* workspace, void* stream_) {
    g_err[0] = 0;
    const long long P = (long long)rays_per_image;
    if (int rc = check_rays_cfg(cfg, P, who)) return rc;
    if (int rc = check_rays(rays, who)) return rc;
    const float *near, *far;
    if (int rc = ray_bounds_of(bounds, who, near, far)) return rc;
    if ((!vols && !no_volume(cfg)) || !packed || !pixels || !dist || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument", who);
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "%s: FiLM layers need freq and phase", who);
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    rng = rng_or_none(rng);
    if (hier && !rng->u_fine && !cfg->philox) return fail(CNERF_EINVAL, "%s: hierarchical sampling needs rng.u_fine (or cfg.philox)", who);
    hipStream_t stream = (hipStream_t)stream_;

    const int S = cfg->S;
    const long long n_rays = (long long)cfg->B * P, npi = P * S;
    const RaysForwardLayout F = rays_forward_layout(cfg, P);
    char* ws = (char*)workspace;
    float* c_rs = (float*)(ws + F.c_rs);
    float* f_rs = (float*)(ws + F.f_rs);
    float* c_z = (float*)(ws + F.c_z);
    float* f_z = (float*)(ws + F.f_z);
    float* c_pts = (float*)(ws + F.pts);
    float* f_pts = c_pts;
    if (aux) {   // write straight into the caller's buffers where given
        if (aux->coarse_rgb_sigma) c_rs = aux->coarse_rgb_sigma;
        if (aux->fine_rgb_sigma) f_rs = aux->fine_rgb_sigma;
        if (aux->coarse_z) c_z = aux->coarse_z;
        if (aux->fine_z) f_z = aux->fine_z;
        if (aux->coarse_points) c_pts = aux->coarse_points;
        if (aux->fine_points) f_pts = aux->fine_points;
    }
    // both field passes: the network at explicit points, no dropout (refused above)
    FieldArgs fa;
    if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, c_pts, 0, cfg->B, npi, nullptr)) return rc;

    // 1. coarse pass: stratified depths and positions, the field
    RaySampleArgs sa{rays->origins, rays->dirs, nullptr, rng->u_strat, c_z, c_pts, n_rays, S, cfg->ray_start, cfg->ray_end, philox_of(cfg), near, far};
    if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, "ray_sample (coarse)");
    fa.rgb_sigma = c_rs;
    if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, "field kernel (coarse)");
    if (hier) {
        // 2. coarse weights -> inverse-CDF depths
        ResampleArgs ra{c_z, nullptr, c_rs, rng->eps_coarse, rng->u_fine, f_z, aux ? aux->inds : nullptr, aux ? aux->cdf : nullptr,
                        aux ? aux->coarse_weights : nullptr, n_rays, S, cfg->noise_std, cfg->flags, philox_of(cfg)};
        if (hipError_t e = launch_resample(ra, stream)) return hip_fail(e, "resample");
        // 3. fine pass
        if (rng->fine_z) f_z = const_cast<float*>(rng->fine_z);   // teacher-forced depths (read only from here on)
        sa.z = f_z;
        sa.u_strat = nullptr;
        sa.z_out = nullptr;
        sa.points = f_pts;
        if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, "ray_sample (fine)");
        fa.points = f_pts;
        fa.rgb_sigma = f_rs;
        if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, "field kernel (fine)");
    }
    // 4. merge + composite, outputs per ray
    MergeArgs ma{c_rs, c_z, hier ? f_rs : nullptr, hier ? f_z : nullptr, rng->eps_final, pixels, dist, aux ? aux->sort_idx : nullptr,
                 aux ? aux->final_weights : nullptr, n_rays, S, RayGeom{}, cfg->noise_std, cfg->flags, philox_of(cfg), 1};
    if (hipError_t e = launch_merge_composite(ma, stream)) return hip_fail(e, "merge_composite");
    return CNERF_OK;
}

int cnerf_render_rays_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_volumes* vols, const float* packed,
                              const float* freq, const float* phase, const cnerf_rng* rng, float* pixels, float* dist, const cnerf_aux* aux,
                              void* workspace, void* stream) {
    return render_rays_forward_impl("render_rays_forward", cfg, rays, rays_per_image, nullptr, vols, packed, freq, phase, rng, pixels, dist, aux, workspace,
                                    stream);
}

int cnerf_render_rays_bounded_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_ray_bounds* bounds,
                                      const cnerf_volumes* vols, const float* packed, const float* freq, const float* phase, const cnerf_rng* rng,
                                      float* pixels, float* dist, const cnerf_aux* aux, void* workspace, void* stream) {
    return render_rays_forward_impl("render_rays_bounded_forward", cfg, rays, rays_per_image, bounds, vols, packed, freq, phase, rng, pixels, dist, aux,
                                    workspace, stream);
}

int cnerf_render_rays_backward_workspace_bytes(const cnerf_cfg* cfg, int32_t backward_precision, int64_t rays_per_image, int64_t points_per_chunk,
                                               size_t* bytes) {
    g_err[0] = 0;
    if (int rc = check_rays_cfg(cfg, (long long)rays_per_image, "render_rays_backward_workspace_bytes")) return rc;
    RaysBackwardLayout R;
    if (int rc = rays_backward_layout(cfg, backward_precision, (long long)rays_per_image, (long long)points_per_chunk, R)) return rc;
    if (bytes) *bytes = R.total;
    return CNERF_OK;
}

int cnerf_render_rays_backward(const cnerf_cfg* cfg, int32_t bprec, int64_t points_per_chunk, const cnerf_rays* rays, int64_t rays_per_image,
                               const cnerf_volumes* vols, const cnerf_field_params* params, const float* packed, const void* packed_bwd,
                               const float* freq, const float* phase, const cnerf_rng* rng, const cnerf_saved* saved, const float* grad_pixels,
                               const float* grad_dist, const cnerf_field_param_grads* grads, float* grad_freq, float* grad_phase,
                               const cnerf_grad_volumes* grad_vols, float* grad_origins, float* grad_dirs, uint32_t* saturated, void* workspace,
                               void* stream_) {
    g_err[0] = 0;
    const long long P = (long long)rays_per_image;
    if (int rc = check_rays_cfg(cfg, P, "render_rays_backward")) return rc;
    if (int rc = check_rays(rays, "render_rays_backward")) return rc;
    RaysBackwardLayout R;
    if (int rc = rays_backward_layout(cfg, bprec, P, (long long)points_per_chunk, R)) return rc;
    if (!saved || !grad_pixels || !workspace) return fail(CNERF_EINVAL, "render_rays_backward: NULL argument");
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    if (!saved->coarse_rgb_sigma || !saved->coarse_z || (hier && (!saved->fine_rgb_sigma || !saved->fine_z)))
        return fail(CNERF_EINVAL, "render_rays_backward: saved rgb_sigma / z of the forward are incomplete");
    const int S = cfg->S;
    const long long n_rays = (long long)cfg->B * P, npi = P * S;
    char* ws = (char*)workspace;
    float* gc = (float*)(ws + R.gc);
    float* gf = hier ? (float*)(ws + R.gf) : nullptr;
    float* pts = (float*)(ws + R.pts);
    float* gpts = grad_origins || grad_dirs ? (float*)(ws + R.gpts) : nullptr;
    // every refusal of the field passes before the first launch
    if (int rc = query_backward(true, cfg, bprec, points_per_chunk, vols, params, packed, packed_bwd, freq, phase, pts, npi, saved->coarse_rgb_sigma, gc, grads,
                                grad_freq, grad_phase, grad_vols, gpts, saturated, ws + R.query, stream_))
        return rc;
    rng = rng_or_none(rng);
    hipStream_t stream = (hipStream_t)stream_;

    // 1. d(pixels, dist) -> d(rgb_sigma) of every coarse / fine sample
    MergeBwdArgs mb{saved->coarse_rgb_sigma, saved->coarse_z, hier ? saved->fine_rgb_sigma : nullptr, hier ? saved->fine_z : nullptr,
                    cfg->noise_std != 0.0f ? rng->eps_final : nullptr, grad_pixels, grad_dist, gc, gf, n_rays, S, RayGeom{}, cfg->noise_std, cfg->flags,
                    philox_of(cfg), 1};
    if (hipError_t e = launch_merge_composite_backward(mb, stream)) return hip_fail(e, "merge_composite_backward");
    // 2. per pass: the sample positions again from the forward's depths, the field query's backward on them (chunked by points_per_chunk),
    //    the position gradients reduced onto the rays -- coarse samples first, then the fine ones
    for (int pass = 0; pass < (hier ? 2 : 1); ++pass) {
        const float* z = pass ? saved->fine_z : saved->coarse_z;
        RaySampleArgs sa{rays->origins, rays->dirs, z, nullptr, nullptr, pts, n_rays, S, cfg->ray_start, cfg->ray_end, philox_of(cfg)};
        if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, "ray_sample");
        if (gpts)
            if (hipError_t e = hipMemsetAsync(gpts, 0, (size_t)n_rays * S * 3 * sizeof(float), stream)) return hip_fail(e, "memset");
        if (int rc = query_backward(false, cfg, bprec, points_per_chunk, vols, params, packed, packed_bwd, freq, phase, pts, npi,
                                    pass ? saved->fine_rgb_sigma : saved->coarse_rgb_sigma, pass ? gf : gc, grads, grad_freq, grad_phase, grad_vols, gpts,
                                    saturated, ws + R.query, stream_))
            return rc;
        if (gpts) {
            RayGradArgs rg{gpts, z, grad_origins, grad_dirs, n_rays, S};
            if (hipError_t e = launch_ray_grad_reduce(rg, stream)) return hip_fail(e, "ray_grad_reduce");
        }
    }
    return CNERF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// occupancy grids: forward-only ray renders that skip empty space (csrc/occupancy.hip)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_occ_shape(int G, const char* who) {
    if (G < 4 || G > 256 || G % 4 != 0) return fail(CNERF_EINVAL, "%s: G=%d must be a multiple of 4 in [4,256]", who, G);
    return CNERF_OK;
}
int check_occ_points(int B, long long n, const char* who) {
    if (B < 1 || B > 65535) return fail(CNERF_EINVAL, "%s: B=%d out of range [1,65535]", who, B);
    if (n < 1 || n > 2147483647LL) return fail(CNERF_EINVAL, "%s: n_per_image=%lld out of range [1,2^31)", who, n);
    return CNERF_OK;
}
int occ_grid(const cnerf_occupancy* occ, const char* who, OccGrid& g) {
    if (!occ) return fail(CNERF_EINVAL, "%s: occupancy is NULL", who);
    if (int rc = check_occ_shape(occ->G, who)) return rc;
    if (!(occ->side > 0.0f) || !(occ->side < INFINITY)) return fail(CNERF_EINVAL, "%s: occupancy side=%g must be > 0 and finite", who, (double)occ->side);
    if (!occ->bits) return fail(CNERF_EINVAL, "%s: occupancy bits is NULL", who);
    g.bits = occ->bits;
    g.G = occ->G;
    for (int k = 0; k < 3; ++k) g.lo[k] = occ->lo[k];
    g.inv = (float)occ->G / occ->side;
    return CNERF_OK;
}
size_t occ_compact_bytes(int B, long long n) { return align256((size_t)B * (size_t)occ_chunks(n) * sizeof(int32_t)); }

// Workspace of cnerf_render_rays_masked_forward: that of cnerf_render_rays_forward, then of the pass in flight the live positions (N, 3),
// their values (N, 4), the ranks (N) int32, the B counts and the compaction's scratch; N = B P S
struct MaskedLayout {
    RaysForwardLayout F;
    size_t live_pts, live_rs, rank, counts, compact, total;
};
MaskedLayout masked_layout(const cnerf_cfg* c, long long P) {
    MaskedLayout M{};
    M.F = rays_forward_layout(c, P);
    const size_t N = (size_t)c->B * (size_t)P * c->S;
    size_t off = M.F.total;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    M.live_pts = take(N * 3 * sizeof(float));
    M.live_rs = take(N * 4 * sizeof(float));
    M.rank = take(N * sizeof(int32_t));
    M.counts = take((size_t)c->B * sizeof(int32_t));
    M.compact = take(occ_compact_bytes(c->B, P * c->S));
    M.total = off;
    return M;
}
}  // namespace

extern "C" {

int cnerf_occupancy_build(int32_t B, int32_t G, int32_t dilate, float threshold, const float* sigma, uint32_t* bits, void* stream) {
    g_err[0] = 0;
    if (int rc = check_occ_shape(G, "occupancy_build")) return rc;
    if (B < 1 || B > 65535) return fail(CNERF_EINVAL, "occupancy_build: B=%d out of range [1,65535]", B);
    if (dilate < 0 || dilate > 4) return fail(CNERF_EINVAL, "occupancy_build: dilate=%d out of range [0,4]", dilate);
    if (!sigma || !bits) return fail(CNERF_EINVAL, "occupancy_build: NULL argument");
    if ((uintptr_t)bits % 8) return fail(CNERF_EINVAL, "occupancy_build: bits must be 8-byte aligned");
    if (hipError_t e = launch_occ_build(OccBuildArgs{sigma, bits, B, G, dilate, threshold}, (hipStream_t)stream)) return hip_fail(e, "occ_build");
    return CNERF_OK;
}

int cnerf_occupancy_compact_bytes(int32_t B, int64_t n_per_image, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_occ_points(B, (long long)n_per_image, "occupancy_compact_bytes")) return rc;
    if (workspace) *workspace = occ_compact_bytes(B, (long long)n_per_image);
    return CNERF_OK;
}

int cnerf_occupancy_compact(const cnerf_occupancy* occ, int32_t B, int64_t n_per_image, const float* points, int32_t* rank, float* live_points,
                            int32_t* counts, void* workspace, void* stream) {
    g_err[0] = 0;
    OccGrid g;
    if (int rc = occ_grid(occ, "occupancy_compact", g)) return rc;
    if (int rc = check_occ_points(B, (long long)n_per_image, "occupancy_compact")) return rc;
    if (!points || !rank || !live_points || !counts || !workspace) return fail(CNERF_EINVAL, "occupancy_compact: NULL argument");
    const OccCompactArgs a{g, points, rank, live_points, counts, (int32_t*)workspace, (long long)n_per_image, B};
    if (hipError_t e = launch_occ_compact(a, (hipStream_t)stream)) return hip_fail(e, "occ_compact");
    return CNERF_OK;
}

int cnerf_occupancy_expand(int32_t B, int64_t n_per_image, const int32_t* rank, const float* live_rgb_sigma, float* rgb_sigma, void* stream) {
    g_err[0] = 0;
    if (int rc = check_occ_points(B, (long long)n_per_image, "occupancy_expand")) return rc;
    if (!rank || !live_rgb_sigma || !rgb_sigma) return fail(CNERF_EINVAL, "occupancy_expand: NULL argument");
    if ((uintptr_t)live_rgb_sigma % 16 || (uintptr_t)rgb_sigma % 16) return fail(CNERF_EINVAL, "occupancy_expand: rgb_sigma buffers must be 16-byte aligned");
    if (live_rgb_sigma == rgb_sigma) return fail(CNERF_EINVAL, "occupancy_expand: live_rgb_sigma and rgb_sigma must be distinct buffers");
    if (hipError_t e = launch_occ_expand(OccExpandArgs{rank, live_rgb_sigma, rgb_sigma, (long long)n_per_image, B}, (hipStream_t)stream))
        return hip_fail(e, "occ_expand");
    return CNERF_OK;
}

int cnerf_render_rays_masked_workspace_bytes(const cnerf_cfg* cfg, int64_t rays_per_image, size_t* bytes) {
    g_err[0] = 0;
    if (int rc = check_rays_cfg(cfg, (long long)rays_per_image, "render_rays_masked_workspace_bytes")) return rc;
    if (int rc = check_occ_points(cfg->B, (long long)rays_per_image * cfg->S, "render_rays_masked_workspace_bytes")) return rc;
    if (bytes) *bytes = masked_layout(cfg, (long long)rays_per_image).total;
    return CNERF_OK;
}

// cnerf_render_rays_masked_forward and cnerf_render_rays_bounded_masked_forward (bounds == NULL: the scalars of cfg)
static int render_rays_masked_forward_impl(const char* who, const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image,
                                           const cnerf_ray_bounds* bounds, const cnerf_occupancy* occ, const cnerf_volumes* vols, const float* packed,
                                           const float* freq, const float* phase, const cnerf_rng* rng, float* pixels, float* dist, const cnerf_aux* aux,
                                           int32_t* live_counts, void* workspace, void* stream_) {
    g_err[0] = 0;
    const long long P = (long long)rays_per_image;
    if (int rc = check_rays_cfg(cfg, P, who)) return rc;
    if (int rc = check_rays(rays, who)) return rc;
    const float *near, *far;
    if (int rc = ray_bounds_of(bounds, who, near, far)) return rc;
    OccGrid grid;
    if (int rc = occ_grid(occ, who, grid)) return rc;
    const int S = cfg->S, B = cfg->B;
    const long long n_rays = (long long)B * P, npi = P * S;
    if (int rc = check_occ_points(B, npi, who)) return rc;
    if ((!vols && !no_volume(cfg)) || !packed || !pixels || !dist || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument", who);
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "%s: FiLM layers need freq and phase", who);
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    rng = rng_or_none(rng);
    if (hier && !rng->u_fine && !cfg->philox) return fail(CNERF_EINVAL, "%s: hierarchical sampling needs rng.u_fine (or cfg.philox)", who);
    hipStream_t stream = (hipStream_t)stream_;
    // the live counts come back to the host between the compaction and the field launches: not something a graph can record
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipError_t e = hipStreamIsCapturing(stream, &capturing)) return hip_fail(e, "hipStreamIsCapturing");
    if (capturing != hipStreamCaptureStatusNone)
        return fail(CNERF_EINVAL, "%s: the stream is being captured; this call copies the live counts to the host and synchronises", who);

    const MaskedLayout M = masked_layout(cfg, P);
    char* ws = (char*)workspace;
    float* c_rs = (float*)(ws + M.F.c_rs);
    float* f_rs = (float*)(ws + M.F.f_rs);
    float* c_z = (float*)(ws + M.F.c_z);
    float* f_z = (float*)(ws + M.F.f_z);
    float* c_pts = (float*)(ws + M.F.pts);
    float* f_pts = c_pts;
    if (aux) {   // write straight into the caller's buffers where given
        if (aux->coarse_rgb_sigma) c_rs = aux->coarse_rgb_sigma;
        if (aux->fine_rgb_sigma) f_rs = aux->fine_rgb_sigma;
        if (aux->coarse_z) c_z = aux->coarse_z;
        if (aux->fine_z) f_z = aux->fine_z;
        if (aux->coarse_points) c_pts = aux->coarse_points;
        if (aux->fine_points) f_pts = aux->fine_points;
    }
    float* live_pts = (float*)(ws + M.live_pts);
    float* live_rs = (float*)(ws + M.live_rs);
    int32_t* rank = (int32_t*)(ws + M.rank);
    int32_t* counts = (int32_t*)(ws + M.counts);
    // every refusal of the field passes before the first launch (the arguments of image 0 stand for all)
    FieldArgs fa;
    if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, live_pts, 0, 1, npi, nullptr)) return rc;
    int32_t* own_counts = live_counts ? nullptr : (int32_t*)malloc((size_t)B * sizeof(int32_t));
    if (!live_counts && !own_counts) return fail(CNERF_EINVAL, "%s: out of host memory", who);

    // one field pass on the live points of `pts`: compact, counts to the host, the field per image, expand into rs
    auto field_pass = [&](const float* pts, float* rs, int32_t* host_counts, const char* what) -> int {
        const OccCompactArgs ca{grid, pts, rank, live_pts, counts, (int32_t*)(ws + M.compact), npi, B};
        if (hipError_t e = launch_occ_compact(ca, stream)) return hip_fail(e, "occ_compact");
        if (hipError_t e = hipMemcpyAsync(host_counts, counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, stream)) return hip_fail(e, "live counts");
        if (hipError_t e = hipStreamSynchronize(stream)) return hip_fail(e, "live counts");
        for (int b = 0; b < B; ++b) {
            if (host_counts[b] <= 0) continue;
            if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, live_pts + (size_t)b * npi * 3, b, 1, host_counts[b], nullptr)) return rc;
            fa.rgb_sigma = live_rs + (size_t)b * npi * 4;
            if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, what);
        }
        if (hipError_t e = launch_occ_expand(OccExpandArgs{rank, live_rs, rs, npi, B}, stream)) return hip_fail(e, "occ_expand");
        return CNERF_OK;
    };
    auto run = [&]() -> int {
        int32_t* hc = live_counts ? live_counts : own_counts;
        // 1. coarse pass: stratified depths and positions, the field on the live ones
        RaySampleArgs sa{rays->origins, rays->dirs, nullptr, rng->u_strat, c_z, c_pts, n_rays, S, cfg->ray_start, cfg->ray_end, philox_of(cfg), near, far};
        if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, "ray_sample (coarse)");
        if (int rc = field_pass(c_pts, c_rs, hc, "field kernel (coarse)")) return rc;
        if (hier) {
            // 2. coarse weights -> inverse-CDF depths
            ResampleArgs ra{c_z, nullptr, c_rs, rng->eps_coarse, rng->u_fine, f_z, aux ? aux->inds : nullptr, aux ? aux->cdf : nullptr,
                            aux ? aux->coarse_weights : nullptr, n_rays, S, cfg->noise_std, cfg->flags, philox_of(cfg)};
            if (hipError_t e = launch_resample(ra, stream)) return hip_fail(e, "resample");
            // 3. fine pass
            if (rng->fine_z) f_z = const_cast<float*>(rng->fine_z);   // teacher-forced depths (read only from here on)
            sa.z = f_z;
            sa.u_strat = nullptr;
            sa.z_out = nullptr;
            sa.points = f_pts;
            if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, "ray_sample (fine)");
            if (int rc = field_pass(f_pts, f_rs, live_counts ? live_counts + B : own_counts, "field kernel (fine)")) return rc;
        }
        // 4. merge + composite, outputs per ray
        MergeArgs ma{c_rs, c_z, hier ? f_rs : nullptr, hier ? f_z : nullptr, rng->eps_final, pixels, dist, aux ? aux->sort_idx : nullptr,
                     aux ? aux->final_weights : nullptr, n_rays, S, RayGeom{}, cfg->noise_std, cfg->flags, philox_of(cfg), 1};
        if (hipError_t e = launch_merge_composite(ma, stream)) return hip_fail(e, "merge_composite");
        return CNERF_OK;
    };
    const int rc = run();
    free(own_counts);
    return rc;
}

int cnerf_render_rays_masked_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_occupancy* occ,
                                     const cnerf_volumes* vols, const float* packed, const float* freq, const float* phase, const cnerf_rng* rng,
                                     float* pixels, float* dist, const cnerf_aux* aux, int32_t* live_counts, void* workspace, void* stream) {
    return render_rays_masked_forward_impl("render_rays_masked_forward", cfg, rays, rays_per_image, nullptr, occ, vols, packed, freq, phase, rng, pixels, dist,
                                           aux, live_counts, workspace, stream);
}

int cnerf_render_rays_bounded_masked_forward(const cnerf_cfg* cfg, const cnerf_rays* rays, int64_t rays_per_image, const cnerf_ray_bounds* bounds,
                                             const cnerf_occupancy* occ, const cnerf_volumes* vols, const float* packed, const float* freq,
                                             const float* phase, const cnerf_rng* rng, float* pixels, float* dist, const cnerf_aux* aux,
                                             int32_t* live_counts, void* workspace, void* stream) {
    return render_rays_masked_forward_impl("render_rays_bounded_masked_forward", cfg, rays, rays_per_image, bounds, occ, vols, packed, freq, phase, rng, pixels,
                                           dist, aux, live_counts, workspace, stream);
}

int cnerf_occupancy_ray_bounds(const cnerf_occupancy* occ, const cnerf_rays* rays, int32_t B, int64_t rays_per_image, float t_min, float t_max, float pad,
                               float* near, float* far, uint8_t* hit, void* stream) {
    g_err[0] = 0;
    const char* who = "occupancy_ray_bounds";
    OccGrid g;
    if (int rc = occ_grid(occ, who, g)) return rc;
    if (int rc = check_rays(rays, who)) return rc;
    if (B < 1 || B > 65535) return fail(CNERF_EINVAL, "%s: B=%d out of range [1,65535]", who, B);
    if (rays_per_image < 1 || rays_per_image > (1LL << 38) / B)       // one lane per ray, 256 per block: at most 2^30 blocks
        return fail(CNERF_EINVAL, "%s: rays_per_image=%lld must be >= 1 (and B * rays_per_image <= 2^38)", who, (long long)rays_per_image);
    if (!(fabsf(t_min) < INFINITY) || !(fabsf(t_max) < INFINITY)) return fail(CNERF_EINVAL, "%s: t_min=%g and t_max=%g must be finite", who, (double)t_min, (double)t_max);
    if (!(t_min < t_max)) return fail(CNERF_EINVAL, "%s: t_max=%g must be greater than t_min=%g", who, (double)t_max, (double)t_min);
    if (!(pad >= 0.0f) || !(pad < INFINITY)) return fail(CNERF_EINVAL, "%s: pad=%g must be >= 0 and finite", who, (double)pad);
    if (!near || !far) return fail(CNERF_EINVAL, "%s: near / far is NULL", who);
    const OccBoundsArgs a{g, occ->side / (float)occ->G, rays->origins, rays->dirs, near, far, hit, (long long)rays_per_image, B, t_min, t_max, pad};
    if (hipError_t e = launch_occ_ray_bounds(a, (hipStream_t)stream)) return hip_fail(e, "occ_ray_bounds");
    return CNERF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// isosurfaces: marching tetrahedra on a scalar lattice (csrc/isosurface.hip)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_iso_shape(int n0, int n1, int n2, const char* who) {
    const int n[3] = {n0, n1, n2};
    for (int c = 0; c < 3; ++c)
        if (n[c] < 2 || n[c] > 1024) return fail(CNERF_EINVAL, "%s: n%d=%d out of range [2,1024]", who, c, n[c]);
    if ((long long)n0 * n1 * n2 > (1LL << 27)) return fail(CNERF_EINVAL, "%s: n0 n1 n2 = %lld exceeds 2^27", who, (long long)n0 * n1 * n2);
    return CNERF_OK;
}
// Workspace of cnerf_isosurface_count / _emit: code (n) uint8, voff (n) int32, toff (n) int32, block sums (2, blocks) int32
struct IsoLayout {
    size_t code, voff, toff, sums, total;
};
IsoLayout iso_layout(const IsoDims& d) {
    IsoLayout W{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
    W.code = take((size_t)d.n);
    W.voff = take((size_t)d.n * sizeof(int32_t));
    W.toff = take((size_t)d.n * sizeof(int32_t));
    W.sums = take((size_t)2 * d.blocks * sizeof(int32_t));
    W.total = off;
    return W;
}
}  // namespace

extern "C" {

int cnerf_isosurface_bytes(int32_t n0, int32_t n1, int32_t n2, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_iso_shape(n0, n1, n2, "isosurface_bytes")) return rc;
    if (workspace) *workspace = iso_layout(iso_dims(n0, n1, n2)).total;
    return CNERF_OK;
}

int cnerf_isosurface_count(int32_t n0, int32_t n1, int32_t n2, const float* values, float level, int32_t* counts, void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "isosurface_count";
    if (int rc = check_iso_shape(n0, n1, n2, who)) return rc;
    if (!values || !counts || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument (values / counts / workspace)", who);
    if (!(fabsf(level) < INFINITY)) return fail(CNERF_EINVAL, "%s: level=%g must be finite", who, (double)level);
    const IsoDims d = iso_dims(n0, n1, n2);
    const IsoLayout W = iso_layout(d);
    char* ws = (char*)workspace;
    const IsoCountArgs a{d, values, level, (uint8_t*)(ws + W.code), (int32_t*)(ws + W.voff), (int32_t*)(ws + W.toff), (int32_t*)(ws + W.sums), counts};
    if (hipError_t e = launch_iso_count(a, (hipStream_t)stream)) return hip_fail(e, "iso_count");
    return CNERF_OK;
}

int cnerf_isosurface_emit(int32_t n0, int32_t n1, int32_t n2, const float* values, float level, const float lo[3], float pitch, const float* attrs,
                          int32_t n_attr, int64_t max_vertices, int64_t max_triangles, float* vertices, float* vertex_attrs, int32_t* triangles,
                          const void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "isosurface_emit";
    if (int rc = check_iso_shape(n0, n1, n2, who)) return rc;
    if (!values || !workspace || !vertices || !triangles || !lo) return fail(CNERF_EINVAL, "%s: NULL argument (values / lo / workspace / vertices / triangles)", who);
    if (!(fabsf(level) < INFINITY)) return fail(CNERF_EINVAL, "%s: level=%g must be finite", who, (double)level);
    if (!(pitch > 0.0f) || !(pitch < INFINITY)) return fail(CNERF_EINVAL, "%s: pitch=%g must be > 0 and finite", who, (double)pitch);
    for (int c = 0; c < 3; ++c)
        if (!(fabsf(lo[c]) < INFINITY)) return fail(CNERF_EINVAL, "%s: lo[%d]=%g must be finite", who, c, (double)lo[c]);
    if ((attrs == nullptr) != (vertex_attrs == nullptr)) return fail(CNERF_EINVAL, "%s: attrs and vertex_attrs must both be given, or neither", who);
    if (attrs && (n_attr < 1 || n_attr > 8)) return fail(CNERF_EINVAL, "%s: n_attr=%d out of range [1,8]", who, n_attr);
    if (max_vertices < 0 || max_triangles < 0)
        return fail(CNERF_EINVAL, "%s: max_vertices=%lld and max_triangles=%lld must be >= 0", who, (long long)max_vertices, (long long)max_triangles);
    const IsoDims d = iso_dims(n0, n1, n2);
    const IsoLayout W = iso_layout(d);
    const char* ws = (const char*)workspace;
    const IsoEmitArgs a{d, values, level, {lo[0], lo[1], lo[2]}, pitch, attrs, attrs ? n_attr : 0, (long long)max_vertices, (long long)max_triangles,
                        vertices, vertex_attrs, triangles, (const uint8_t*)(ws + W.code), (const int32_t*)(ws + W.voff), (const int32_t*)(ws + W.toff),
                        (const int32_t*)(ws + W.sums)};
    if (hipError_t e = launch_iso_emit(a, (hipStream_t)stream)) return hip_fail(e, "iso_emit");
    return CNERF_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// nearest points: exact brute-force search between two batched clouds (csrc/nearest.hip)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
constexpr long long NN_FILL_WAVES = 4096;     // work items (one wave each) that fill the card: 256 CUs x 4 SIMDs x 4 waves
constexpr long long NN_MIN_RANGE = 1024;      // targets a range keeps at least, so that a partial per query is paid for
// target_splits == 0: a pure function of (B, n, m)
int nearest_auto_splits(int B, long long n, long long m) {
    const long long items = (long long)B * ((n + NN_QUERIES - 1) / NN_QUERIES);
    long long s = (NN_FILL_WAVES + items - 1) / items;
    const long long cap = (m + NN_MIN_RANGE - 1) / NN_MIN_RANGE;
    if (s > cap) s = cap;
    return (int)(s < 1 ? 1 : (s > 1024 ? 1024 : s));
}
int check_nearest_shape(int B, long long n, long long m, int target_splits, const char* who) {
    if (B < 1) return fail(CNERF_EINVAL, "%s: B=%d must be >= 1", who, B);
    if (n < 1) return fail(CNERF_EINVAL, "%s: n=%lld must be >= 1", who, n);
    if (m < 1 || m >= (1LL << 31)) return fail(CNERF_EINVAL, "%s: m=%lld out of range [1,2^31)", who, m);
    if (n > ((1LL << 40) - 1) / B) return fail(CNERF_EINVAL, "%s: B n = %d x %lld must be below 2^40", who, B, n);
    if (target_splits < 0 || target_splits > 1024) return fail(CNERF_EINVAL, "%s: target_splits=%d out of range [0,1024]", who, target_splits);
    return CNERF_OK;
}
// Workspace of cnerf_nearest_points with S > 1 ranges: partial distances (B,S,n) float, partial indices (B,S,n) int32
struct NearestLayout {
    int splits;
    size_t part_d, part_j, total;
};
NearestLayout nearest_layout(int B, long long n, long long m, int target_splits) {
    NearestLayout W{};
    W.splits = target_splits ? target_splits : nearest_auto_splits(B, n, m);
    if (W.splits > 1) {
        const size_t part = align256((size_t)B * W.splits * n * sizeof(float));
        W.part_j = part;
        W.total = 2 * part;
    }
    return W;
}
}  // namespace

extern "C" {

int cnerf_nearest_points_tiling(int32_t* queries_per_block, int32_t* targets_per_tile) {
    g_err[0] = 0;
    if (queries_per_block) *queries_per_block = NN_QUERIES;
    if (targets_per_tile) *targets_per_tile = NN_TILE;
    return CNERF_OK;
}

int cnerf_nearest_points_bytes(int32_t B, int64_t n, int64_t m, int32_t target_splits, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_nearest_shape(B, (long long)n, (long long)m, target_splits, "nearest_points_bytes")) return rc;
    if (workspace) *workspace = nearest_layout(B, (long long)n, (long long)m, target_splits).total;
    return CNERF_OK;
}

int cnerf_nearest_points(int32_t B, int64_t n, int64_t m, const float* queries, const float* targets, const int32_t* n_queries,
                         const int32_t* n_targets, int32_t target_splits, float* dist2, int32_t* idx, void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "nearest_points";
    if (int rc = check_nearest_shape(B, (long long)n, (long long)m, target_splits, who)) return rc;
    if (!queries || !targets || !dist2 || !idx) return fail(CNERF_EINVAL, "%s: NULL argument (queries / targets / dist2 / idx)", who);
    const NearestLayout W = nearest_layout(B, (long long)n, (long long)m, target_splits);
    if (W.total && !workspace) return fail(CNERF_EINVAL, "%s: workspace is NULL, %zu bytes are needed (cnerf_nearest_points_bytes)", who, W.total);
    char* ws = (char*)workspace;
    const NearestArgs a{B, (long long)n, (long long)m, W.splits, queries, targets, n_queries, n_targets, dist2, idx,
                        W.total ? (float*)(ws + W.part_d) : nullptr, W.total ? (int32_t*)(ws + W.part_j) : nullptr};
    if (hipError_t e = launch_nearest_points(a, (hipStream_t)stream)) return hip_fail(e, "nearest_points");
    return CNERF_OK;
}

}  // extern "C"
