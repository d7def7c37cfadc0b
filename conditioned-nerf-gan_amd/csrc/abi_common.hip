// The C ABI of libcnerf_hip.so (include/cnerf.h, entries in abi_forward / _backward / _rays / _shapes.hip) is host-side only: argument
// validation, buffer carving, launch sequencing on the caller's stream.  No allocation, no synchronisation, no global state -- with one
// exception, stated in the header: cnerf_render_rays_masked_forward reads the live counts of its compactions back and synchronises the
// stream for them.  Here: what abi_common.hpp declares and does not define inline.
#include "abi_common.hpp"

namespace cnerf {

__thread char g_err[256] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

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

int fill_field_args(FieldArgs& a, const cnerf_cfg* c, const cnerf_volumes* vols, const cnerf_grad_volumes* gvols, const float* packed, const float* freq,
                    const float* phase, int image0) {
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

}  // namespace cnerf
