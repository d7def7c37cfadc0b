// What the translation units of the C ABI share (abi_forward.hip, abi_backward.hip, abi_rays.hip, abi_shapes.hip; the entries are declared
// in include/cnerf.h): the error buffer, the checks and counts every path derives from a cfg, the layout of the packed weights, the
// FieldArgs of a field pass, and the one sequence of a forward render.  Host-side only.  What needs one definition is in abi_common.hip.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cnerf_kernels.hpp"

#pragma GCC visibility push(hidden)      // internal to libcnerf_hip.so: the error buffer above all is one object, and no export
namespace cnerf {

// the message cnerf_last_error returns (per thread; every entry clears it first).  __thread: plain storage without the initialisation
// wrapper a thread_local declared in one translation unit and defined in another is read through
extern __thread char g_err[256];
int fail(int code, const char* fmt, ...);
inline int hip_fail(hipError_t e, const char* what) { return fail(CNERF_ELAUNCH, "%s: %s", what, hipGetErrorString(e)); }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves a workspace into 256-byte aligned pieces: take() returns the offset of the next piece, `off` ends as the total
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align256(bytes); return o; }
};

// CNERF_F_NO_VOLUME: no feature volume, layer 0 reads the sample position
inline bool no_volume(const cnerf_cfg* c) { return (c->flags & CNERF_F_NO_VOLUME) != 0; }

int check_cfg(const cnerf_cfg* c, bool need_render);

inline int n_levels_of(const cnerf_cfg* c) { return c->n_levels > 0 ? c->n_levels : (no_volume(c) ? 0 : 1); }
inline int level_V_of(const cnerf_cfg* c, int i) { return c->n_levels > 0 ? c->level_V[i] : c->V; }
inline int level_C_of(const cnerf_cfg* c, int i) { return c->n_levels > 0 ? c->level_C[i] : c->C; }
// floats of one image's volume level i (V^3 C, channel-last)
inline size_t level_floats(const cnerf_cfg* c, int i) { const size_t V = level_V_of(c, i); return V * V * V * level_C_of(c, i); }

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
inline NetCounts counts_of(const cnerf_cfg* c) {
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
PackedLayout packed_layout(const cnerf_cfg* c);

inline PhiloxKey philox_of(const cnerf_cfg* c) {
    return PhiloxKey{c->philox ? 1u : 0u, c->philox_offset, (uint32_t)(c->philox_seed & 0xffffffffull), (uint32_t)(c->philox_seed >> 32)};
}

inline RayGeom make_geom(const cnerf_cfg* c) {
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
int fill_field_args(FieldArgs& a, const cnerf_cfg* c, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols, const float* packed, const float* freq,
                    const float* phase, int image0 = 0);

// which keep decisions a pass uses: the injected bytes, or Philox stream `stream_id` (fill_field_args set the rest)
inline void set_dropout(FieldArgs& a, const cnerf_cfg* c, const uint8_t* mask, uint32_t stream_id, long long n_per_image) {
    a.drop_mask = c->drop_p > 0.0f ? mask : nullptr;
    a.drop_stream = stream_id;
    a.drop_points = (long long)c->B * n_per_image;
}

inline hipError_t launch_forward(const FieldArgs& a, const cnerf_cfg* c, hipStream_t stream) {
    if (c->layer_kind[0] == CNERF_LAYER_PFILM && c->precision != CNERF_PREC_FP32)
        return c->precision == CNERF_PREC_FP16 ? launch_field_pw1(a, c->H, stream) : launch_field_pw3(a, c->H, stream);
    if (c->precision == CNERF_PREC_FP16X3) return launch_field_h3(a, c->H, stream);
    if (c->precision == CNERF_PREC_FP16) return launch_field_h1(a, c->H, stream);
    return launch_field(a, c->H, stream);
}

inline void set_points(FieldArgs& a, int B, long long n_per_image) {
    a.n_per_image = n_per_image;
    a.tiles_per_image = (n_per_image + 31) / 32;
    a.total_tiles = a.tiles_per_image * B;
}

// FieldArgs of explicit points: n_images images from image0 of the call, n_per_image positions each (`points`: the first image's), the
// keep decisions of dropout stream PHILOX_DROP_POINTS (`mask`, or Philox when NULL)
inline int points_args(FieldArgs& a, const cnerf_cfg* c, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols, const float* packed, const float* freq,
                const float* phase, const float* points, int image0, int n_images, long long n_per_image, const uint8_t* mask) {
    if (int rc = fill_field_args(a, c, vols, gvols, packed, freq, phase, image0)) return rc;
    a.mode = FIELD_MODE_POINTS;
    a.points = points;
    set_points(a, n_images, n_per_image);
    set_dropout(a, c, mask, PHILOX_DROP_POINTS, n_per_image);
    return CNERF_OK;
}

// the draws of a call that passes no cnerf_rng: none
inline const cnerf_rng* rng_or_none(const cnerf_rng* rng) {
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
inline int matrix_set(const cnerf_cfg* cfg, const cnerf_field_params* P, const cnerf_field_param_grads* G, const char* who, MatrixSet& ms) {
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

// cnerf_field_query_backward (abi_backward.hip), which a ray render's backward runs per pass.  check_only: every refusal and no launch
// (points, saved_rgb_sigma, grad_rgb_sigma, workspace: any non-NULL placeholders then)
int query_backward(bool check_only, const cnerf_cfg* cfg, int32_t bprec, int64_t points_per_chunk, const cnerf_volumes* vols, const cnerf_field_params* P,
                   const float* packed, const void* packed_bwd, const float* freq, const float* phase, const float* points, int64_t n_per_image,
                   const float* saved_rgb_sigma, const float* grad_rgb_sigma, const cnerf_field_param_grads* G, float* grad_freq, float* grad_phase,
                   const cnerf_grad_volumes* grad_vols, float* grad_points, uint32_t* saturated, void* workspace, void* stream_);

// ---------------------------------------------------------------------------------------------------------------------
// the forward render: cnerf_render_forward on the R x R grid, the ray batches, the occupancy-masked ray batches
// ---------------------------------------------------------------------------------------------------------------------
// The refusals the renders share, after the driver's own: NULL arguments (inputs_given: the driver's own inputs), FiLM rows, the draws of
// hierarchical sampling.  A NULL rng becomes the one without draws.
inline int check_render(const char* who, const cnerf_cfg* cfg, bool inputs_given, const cnerf_volumes* vols, const float* packed, const float* freq,
                 const float* phase, const float* pixels, const float* depth, const void* workspace, const cnerf_rng*& rng) {
    if (!inputs_given || (!vols && !no_volume(cfg)) || !packed || !pixels || !depth || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument", who);
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "%s: FiLM layers need freq and phase", who);
    rng = rng_or_none(rng);
    if ((cfg->flags & CNERF_F_HIERARCHICAL) && !rng->u_fine && !cfg->philox)
        return fail(CNERF_EINVAL, "%s: hierarchical sampling needs rng.u_fine (or cfg.philox)", who);
    return CNERF_OK;
}

// Buffers of the two passes: rgb_sigma (N, 4), depths (N), sample positions (N, 3) -- the grid render keeps none unless aux asks
struct RenderBuffers { float *c_rs, *f_rs, *c_z, *f_z, *c_pts, *f_pts; };

// coarse field pass -> resample -> fine field pass -> merge + composite + epilogue, on `b` (the driver's workspace pieces) or the caller's
// aux buffers where given.  field_pass(fine, b): the driver's pass -- coarse: depths into b.c_z, values into b.c_rs (positions: b.c_pts);
// fine: values at the depths b.f_z into b.f_rs (b.f_pts).  geom / per_ray: the merge's output layout (MergeArgs).  Every refusal of the
// driver and of its passes comes before this.
template <class FieldPass>
int render_sequence(const cnerf_cfg* cfg, long long n_rays, const cnerf_rng* rng, const cnerf_aux* aux, RenderBuffers b, const RayGeom& geom, int per_ray,
                    float* pixels, float* depth, FieldPass&& field_pass, hipStream_t stream) {
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    if (aux) {   // write straight into the caller's buffers where given
        if (aux->coarse_rgb_sigma) b.c_rs = aux->coarse_rgb_sigma;
        if (aux->fine_rgb_sigma) b.f_rs = aux->fine_rgb_sigma;
        if (aux->coarse_z) b.c_z = aux->coarse_z;
        if (aux->fine_z) b.f_z = aux->fine_z;
        if (aux->coarse_points) b.c_pts = aux->coarse_points;
        if (aux->fine_points) b.f_pts = aux->fine_points;
    }
    // 1. coarse pass
    if (int rc = field_pass(false, b)) return rc;
    if (hier) {
        // 2. coarse weights -> inverse-CDF depths
        ResampleArgs ra{b.c_z, nullptr, b.c_rs, rng->eps_coarse, rng->u_fine, b.f_z, aux ? aux->inds : nullptr, aux ? aux->cdf : nullptr,
                        aux ? aux->coarse_weights : nullptr, n_rays, cfg->S, cfg->noise_std, cfg->flags, philox_of(cfg)};
        if (hipError_t e = launch_resample(ra, stream)) return hip_fail(e, "resample");
        // 3. fine pass
        if (rng->fine_z) b.f_z = const_cast<float*>(rng->fine_z);   // teacher-forced depths (read only from here on)
        if (int rc = field_pass(true, b)) return rc;
    }
    // 4. merge + composite + epilogue
    MergeArgs ma{b.c_rs, b.c_z, hier ? b.f_rs : nullptr, hier ? b.f_z : nullptr, rng->eps_final, pixels, depth, aux ? aux->sort_idx : nullptr,
                 aux ? aux->final_weights : nullptr, n_rays, cfg->S, geom, cfg->noise_std, cfg->flags, philox_of(cfg), per_ray};
    if (hipError_t e = launch_merge_composite(ma, stream)) return hip_fail(e, "merge_composite");
    return CNERF_OK;
}

}  // namespace cnerf
#pragma GCC visibility pop
