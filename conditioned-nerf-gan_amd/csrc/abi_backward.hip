// C ABI (include/cnerf.h), backward side: the backward stages, transposed and half-precision weight packing, weight gradients, the
// scatter entries, cnerf_render_backward in one call, the gradients of a field query, the mapping-network stage of per-point FiLM.
#include "abi_common.hpp"

using namespace cnerf;

namespace {
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

// the activation-storing re-run of a half-precision backward: the pass `a` again, storing fp16 TB16 activations (amax: per-point FiLM
// family only); its head output goes to `rgb_sigma`, (n,4) floats: the stage entries hand it to the caller (it equals the non-storing
// kernel's), the chunk drivers point it at a workspace buffer nobody reads -- the chain overwrites that buffer entirely
FieldArgs storing_args(const FieldArgs& a, long long n_points, void* feat, void* h, void* c, float* amax, void* rgb_sigma) {
    FieldArgs s = a;
    s.rgb_sigma = (float*)rgb_sigma;
    s.act_points = n_points;
    s.act_feat = (float*)feat;
    s.act_h = (float*)h;
    s.act_c = (float*)c;
    s.act_amax = amax;
    s.act_tb16 = 1;
    return s;
}

// The storing re-run of a half-precision chunk, FiLM / plain-sine / residual networks (field_h3.hip, STORE_TB16 on the shared weights):
// the chunk's pass `fa` again, leaving its gradient volumes alone.  ONE launch for chunk16 and for the stage entry cnerf_field_store16.
int store16_forward(FieldArgs fa, int H, long long n_points, void* feat, void* h, void* c, void* rgb_sigma, hipStream_t stream) {
    for (float*& g : fa.lvl_grad) g = nullptr;
    fa.gin = nullptr;
    if (hipError_t e = launch_field_h3(storing_args(fa, n_points, feat, h, c, nullptr, rgb_sigma), H, stream))
        return hip_fail(e, "field kernel (fp16 activation store)");
    return CNERF_OK;
}

// The storing forward of a half-precision per-point FiLM chunk (field_pw16.hip: field_pw16_kernel<NT, STORE> for y, cos, m and the input
// tiles, then pw_deriv_kernel for cos f, cos 15 pre and amax): the chunk's pass `fa` again; the kernels read no gradient volume.  ONE
// launch for chunk_pw16 and for the stage entry cnerf_field_store_pw16.
int store_pw16_forward(const FieldArgs& fa, int H, long long n_points, void* feat, void* h, void* c, float* amax, void* rgb_sigma, hipStream_t stream) {
    if (hipError_t e = launch_field_pw3(storing_args(fa, n_points, feat, h, c, amax, rgb_sigma), H, stream))
        return hip_fail(e, "field kernel (fp16 activation store)");
    return CNERF_OK;
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
    Carver w;
    L.gc = w.take(N_out * 4 * sizeof(float));
    L.gf = w.take(hier ? N_out * 4 * sizeof(float) : 0);
    if (pfilm && !half) {       // the chunk matrices of cnerf_field_backward (include/cnerf.h), then what the mapping-network stage needs; it
                                // accumulates straight into the caller's gradients: no per-image reductions
        if (int rc = pfilm_finish_layout(c, cnt, (long long)npi, who, L.F)) return rc;
        L.a_feat = w.take(n * 32 * sizeof(float));
        L.a_h = w.take((Lc * n * H + n * 256) * sizeof(float));
        L.a_c = w.take(3 * Lc * n * H * sizeof(float));
        L.a_g = w.take(3 * Lc * n * H * sizeof(float));
        L.a_go = w.take(n * 4 * sizeof(float));
        L.pts = w.take(render ? n * 3 * sizeof(float) : 0);
        L.fin = w.take(L.F.total);
        L.map = w.take(L.F.packed_map);
        L.total = w.off;
        return CNERF_OK;
    }
    if (pfilm) {      // chain_pw16.hip: three stored derivatives and three gradient slabs per layer, m and g_mpre
        L.a_feat = w.take(have_act16 ? 0 : T * 2 * 2048);
        L.a_h = w.take(have_act16 ? 0 : (Lc * NT + 8) * T * 2048);
        L.a_c = w.take(have_act16 ? 0 : 3 * Lc * NT * T * 2048);
        L.a_amax = w.take(have_act16 ? 0 : Lc * T * 32 * sizeof(float));
        L.a_g = w.take((3 * Lc * NT + 8) * T * 2048);
        L.a_go = w.take(T * 2048);
        L.a_gy = w.take(Lc * NT * T * 2048);                          // two-kernel chain: g_y slabs
        L.gmax = w.take((5 * Lc + 2) * sizeof(uint32_t));             // 3 L + 2 sampled maxima, L of g_y, L of the stored derivatives
        L.scales = w.take((2 * (4 * Lc + 2) + 2 * Lc) * sizeof(float));   // {S, 1 / S} x (4 L + 2), then per layer {r, To}
    } else if (half) {
        L.a_feat = w.take(have_act16 ? 0 : T * L.n_in * 2048);
        L.a_h = w.take(have_act16 ? 0 : (size_t)L.n_mats * T * NT * 2048);
        L.a_c = w.take(have_act16 ? 0 : (size_t)L.n_mats * T * NT * 2048);
        L.a_g = w.take((size_t)L.n_mats * T * NT * 2048);
        L.a_go = w.take(T * 2048);
        L.a_gin = w.take(render && !no_volume(c) ? (size_t)L.n_in * n * 32 * sizeof(float) : 0);   // (no feature tile: no rows, no patch scatter)
    } else {
        L.a_feat = w.take(n * 32 * L.n_in * sizeof(float));
        L.a_h = w.take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_c = w.take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_g = w.take((size_t)L.n_mats * n * H * sizeof(float));
        L.a_go = w.take(n * 4 * sizeof(float));
    }
    if (!pfilm) {
        L.gmax = w.take((size_t)(L.n_mats + 2) * sizeof(uint32_t));
        L.scales = w.take((size_t)2 * (L.n_mats + 1) * sizeof(float));
    }
    const size_t rows = pfilm ? 256 : H, kmax = pfilm ? 256 : 32 * (size_t)(L.n_in > (int)NT ? L.n_in : (int)NT);   // the largest reduced matrix
    L.dwarg = w.take((size_t)cnt * rows * kmax * sizeof(float));
    L.cs = w.take((size_t)cnt * rows * sizeof(float));
    L.dwh = w.take((size_t)cnt * 4 * H * sizeof(float));
    L.csh = w.take((size_t)cnt * 4 * sizeof(float));
    L.total = w.off;
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

// The gradient chain of a half-precision chunk of cnt images of npi points (tpi tiles) each, FiLM / plain-sine / residual networks
// (bwd16.hip), on the caller's buffers: the head's scale from the largest |d loss / d rgb_sigma| of the chunk, the chain's dry run over
// every step-th tile group for the per-slab maxima, their scales, the chain.  ONE sequence for chunk16 and for the stage entry
// cnerf_field_chain16.  fc: the chunk's pass; it adds to its gradient volumes or stores the rows fc.gin.  group_step: 0 = every 16th
// tile group once there are plenty (groups / 2048, clamped to 1..16), k >= 1 = every k-th.  gmax: n_mats + 2 words; scales: 2 (n_mats + 1).
// between(): what the caller launches behind the head's scale and in front of the dry run (chunk16: the storing re-run, where the render
// has always launched it; the stage entry: nothing).
extern "C++" template <class Between>
int chain16_sequence(const cnerf_cfg* cfg, const void* packed_bwd, FieldArgs fc, int cnt, long long npi, long long tpi, const float* g_out,
                     const float* s_out, const void* a_c, void* a_g, void* a_go, uint32_t* gmax, float* scales, int group_step, uint32_t* saturated,
                     hipStream_t stream, Between&& between) {
    const int H = cfg->H;
    Chain16Layout cl;
    if (int rc = chain16_layout(cfg, cl)) return rc;
    const char* base16 = (const char*)packed_bwd;
    const float* winv = (const float*)(base16 + cl.winv_off);
    if (int rc = head_scales(g_out, (long long)cnt * npi * 4, gmax, cl.n_mats + 2, gmax + cl.n_mats + 1, scales, cl.n_mats, stream)) return rc;
    long long step = group_step;
    if (step < 1) {                                       // dry-run sampling: every 16th tile group once there are plenty
        step = (long long)cnt * ((tpi + 3) / 4) / 2048;
        step = step < 1 ? 1 : (step > 16 ? 16 : step);
    }
    if (int rc = between()) return rc;
    // the dry run (fa) leaves the gradient volumes alone; the chain (fc) adds to them
    FieldArgs fa = fc;
    for (float*& g : fa.lvl_grad) g = nullptr;
    fa.gin = nullptr;
    fa.grad_out = fc.grad_out = g_out;
    fa.saved_out = fc.saved_out = s_out;
    if (hipError_t e = launch_chain16(fa, H, base16, base16 + cl.head_off, winv, scales, a_c, nullptr, nullptr, gmax, nullptr, cl.n_mats, 1, (int)step,
                                      stream))
        return hip_fail(e, "chain16 (dry run)");
    if (hipError_t e = launch_pow2_scales(gmax, cl.n_mats, scales, stream)) return hip_fail(e, "pow2_scales");
    if (hipError_t e = launch_chain16(fc, H, base16, base16 + cl.head_off, winv, scales, a_c, a_g, a_go, nullptr, saturated, cl.n_mats, 0, 1, stream))
        return hip_fail(e, "chain16");
    return CNERF_OK;
}

// half precision, FiLM / plain-sine / residual networks (bwd16.hip): the chain's sequence above with the storing re-run (fp16x3 kernel)
// in it unless the activations are given, the patch scatter of the input-tile gradients (fc.gin set), one weight_grad16 per matrix.  fc: the chunk's
// pass with gradient volumes.
int chunk16(const cnerf_cfg* cfg, const MatrixSet& ms, const BackwardLayout& L, char* ws, const void* packed_bwd, FieldArgs fc, const Chunk& k,
            const float* g_out, const float* s_out, void* a_feat, void* a_h, void* a_c, bool store, const float* freq,
            const cnerf_field_param_grads* G, float* grad_freq, float* grad_phase, uint32_t* saturated, hipStream_t stream) {
    const int H = cfg->H, NT = H / 32;
    const long long T = (long long)k.cnt * k.tpi;
    float* scales = (float*)(ws + L.scales);
    char* a_g = ws + L.a_g;
    char* a_go = ws + L.a_go;
    auto store_forward = [&]() -> int {
        return store ? store16_forward(fc, H, (long long)k.cnt * k.npi, a_feat, a_h, a_c, a_g, stream) : (int)CNERF_OK;
    };
    if (int rc = chain16_sequence(cfg, packed_bwd, fc, k.cnt, k.npi, k.tpi, g_out, s_out, a_c, a_g, a_go, (uint32_t*)(ws + L.gmax), scales, 0, saturated,
                                  stream, store_forward))
        return rc;
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

// The two gradient-chain kernels of a half-precision per-point FiLM chunk of cnt images of npi points (tpi tiles) each (chain_pw16.hip), on
// the caller's buffers: the head's scale from the largest |d loss / d rgb_sigma| of the chunk, chain_pre's dry run over every step-th tile
// group for the g_y maxima, their scales, the largest stored derivative per layer (r_l, To_l and the three slab scales), chain_pre; then
// pw_gm's dry run for g_mpre's scale and pw_gm, which adds to fa's gradient volume.  ONE sequence for chunk_pw16 and for the stage entry
// cnerf_field_chain_pw16.  group_step: 0 = groups / 1024 clamped to 1..32 (at least 1024 tile groups -- 131 k points -- are sampled, every
// 32nd at most), k >= 1 = every k-th.  gmax: 5 L + 2 words; scales: 2 (4 L + 2) + 2 L floats, `lay` = {r_l, To_l} per layer at the end.
int chain_pw16_sequence(const cnerf_cfg* cfg, const void* packed_bwd, FieldArgs fa, int cnt, long long npi, long long tpi, const float* g_out,
                        const float* s_out, const void* a_c, const float* a_amax, const void* m16, void* a_gy, void* a_g, void* a_go, uint32_t* gmax,
                        float* scales, int group_step, uint32_t* saturated, hipStream_t stream) {
    const int H = cfg->H, Lc = cfg->L, n_slots = 3 * Lc + 2;
    const long long T = (long long)cnt * tpi;
    const PwChainLayout cl = pw_chain_layout(cfg);
    const char* base16 = (const char*)packed_bwd;
    fa.grad_out = g_out;
    fa.saved_out = s_out;
    if (int rc = head_scales(fa.grad_out, (long long)cnt * npi * 4, gmax, 5 * Lc + 2, gmax + n_slots - 1, scales, n_slots - 1, stream)) return rc;
    float* lay = scales + 2 * (4 * Lc + 2);
    PwChainBuffers cb{base16, base16 + cl.m_off, base16 + cl.head_off, (const float*)(base16 + cl.winv_off), (const float*)(base16 + cl.anorm_off),
                      scales, lay, a_c, a_amax, m16, a_gy, a_g, a_go, gmax, nullptr};
    long long step = group_step;
    if (step < 1) {                                       // dry-run sampling: at least 1024 tile groups (131 k points), every 32nd at most
        step = (long long)cnt * ((tpi + 3) / 4) / 1024;
        step = step < 1 ? 1 : (step > 32 ? 32 : step);
    }
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
    return CNERF_OK;
}

// half precision, per-point FiLM family: storing forward (field_pw16.hip) unless the activations are given, the chain's sequence above
// (chain_pw16.hip), one weight_grad16 reduction per matrix: dW_l = g_pre_l^T y_{l-1}, dWm2 rows = (g_fr_l | g_ph_l)^T m,
// dWm1 = g_mpre^T feat, head.  fa: the chunk's pass with gradient volumes.
int chunk_pw16(const cnerf_cfg* cfg, const BackwardLayout& L, char* ws, const void* packed_bwd, FieldArgs fa, const Chunk& k, const float* g_out,
               const float* s_out, char* a_feat, char* a_h, char* a_c, float* a_amax, bool store, const cnerf_field_param_grads* G, uint32_t* saturated,
               hipStream_t stream) {
    const int H = cfg->H, NT = H / 32, Lc = cfg->L, n_slots = 3 * Lc + 2;
    const long long T = (long long)k.cnt * k.tpi;
    float* scales = (float*)(ws + L.scales);
    char* a_g = ws + L.a_g;
    char* a_go = ws + L.a_go;
    float* dwarg = (float*)(ws + L.dwarg);
    float* cs = (float*)(ws + L.cs);
    if (store)
        if (int rc = store_pw16_forward(fa, H, (long long)k.cnt * k.npi, a_feat, a_h, a_c, a_amax, a_g, stream)) return rc;
    const size_t slabH = (size_t)T * NT * 2048;            // bytes per (tiles, NT, 32, 32) slab
    if (int rc = chain_pw16_sequence(cfg, packed_bwd, fa, k.cnt, k.npi, k.tpi, g_out, s_out, a_c, a_amax, a_h + (size_t)Lc * slabH, ws + L.a_gy, a_g, a_go,
                                     (uint32_t*)(ws + L.gmax), scales, 0, saturated, stream))
        return rc;
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

int cnerf_field_chain16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const void* packed16, const float* freq,
                        const float* cam2world, const float* u_strat, const float* fine_z, const float* grad_rgb_sigma,
                        const float* saved_rgb_sigma, const void* cos16, int32_t group_step, void* g16, void* go16, float* scales, uint32_t* gmax,
                        float* gin, const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM)
        return fail(CNERF_EINVAL, "field_chain16: FiLM / plain-sine / residual layers only (the per-point FiLM family has a chain of its own)");
    if (cfg->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "field_chain16: a stage of the fp16 backward: cfg->precision must be CNERF_PREC_FP16X3");
    if (pass < 0 || pass > 2) return fail(CNERF_EINVAL, "field_chain16: pass must be 0 (coarse), 1 (fine) or 2 (explicit points)");
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "field_chain16: image range out of [0,B)");
    if (group_step < 0) return fail(CNERF_EINVAL, "field_chain16: group_step=%d must be 0 (the render's rule) or >= 1", group_step);
    if (!packed16 || !grad_rgb_sigma || !saved_rgb_sigma || !cos16 || !g16 || !go16 || !scales || !gmax)
        return fail(CNERF_EINVAL, "field_chain16: NULL argument (packed16, grad_rgb_sigma, saved_rgb_sigma, cos16, g16, go16, scales, gmax)");
    if (counts_of(cfg).n_film && !freq) return fail(CNERF_EINVAL, "field_chain16: FiLM layers need freq");
    // the chain forms the sample positions of every tile, whether or not it scatters them itself
    if (pass != 2 && !cam2world) return fail(CNERF_EINVAL, "field_chain16: NULL argument (cam2world of a ray pass)");
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "field_chain16: the fine pass needs fine_z");
    const bool nv = no_volume(cfg);
    if (!nv) {
        if ((gin != nullptr) == (grad_vols != nullptr)) return fail(CNERF_EINVAL, "field_chain16: exactly one of gin and grad_vols receives the layer-0 gradients");
        if (grad_vols)
            if (int rc = check_grad_vols(cfg, grad_vols, "field_chain16")) return rc;
    }
    if (pass == 2 && !u_strat) return fail(CNERF_EINVAL, "field_chain16: pass 2 takes the points (B,R*R*S,3) in the u_strat argument");
    // the chain reads no volume, no forward weights and (explicit points) no camera: packed16 stands in for the addresses pass_args wants
    // to see (it offsets them and dereferences nothing); they are taken out again below
    const float* stand_in = (const float*)packed16;
    cnerf_volumes unread;
    memset(&unread, 0, sizeof(unread));
    for (int i = 0; i < n_levels_of(cfg); ++i) unread.level[i] = stand_in;
    FieldArgs fc;
    if (int rc = pass_args(fc, cfg, pass, image0, n_images, &unread, nv || gin ? nullptr : grad_vols, nullptr, freq, nullptr,
                           pass == 2 ? stand_in : cam2world, u_strat, fine_z))
        return rc;
    for (const float*& v : fc.lvl_vol) v = nullptr;
    if (pass == 2) fc.cam2world = nullptr;
    fc.gin = nv ? nullptr : gin;
    hipStream_t stream = (hipStream_t)stream_;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S, tpi = (npi + 31) / 32;
    // only channels 0..3 of a row of the head gradient are ever written: the rest must read as zero (the render zeroes its buffer once per call)
    if (hipError_t e = hipMemsetAsync(go16, 0, (size_t)n_images * tpi * 2048, stream)) return hip_fail(e, "memset");
    return chain16_sequence(cfg, packed16, fc, n_images, npi, tpi, grad_rgb_sigma + (size_t)image0 * npi * 4, saved_rgb_sigma + (size_t)image0 * npi * 4,
                            cos16, g16, go16, gmax, scales, group_step, saturated, stream, [] { return (int)CNERF_OK; });
}

int cnerf_field_store16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols, const float* packed,
                        const float* freq, const float* phase, const float* cam2world, const float* u_strat, const float* fine_z, void* feat,
                        void* h, void* c, float* rgb_sigma, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;        // (drop_p != 0 with a half-precision cfg is refused here)
    if (cfg->layer_kind[0] == CNERF_LAYER_PFILM)
        return fail(CNERF_EINVAL, "field_store16: FiLM / plain-sine / residual layers only (the per-point FiLM family has a storing forward of its own)");
    if (cfg->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "field_store16: a stage of the fp16 backward: cfg->precision must be CNERF_PREC_FP16X3");
    if (pass < 0 || pass > 2) return fail(CNERF_EINVAL, "field_store16: pass must be 0 (coarse), 1 (fine) or 2 (explicit points)");
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "field_store16: image range out of [0,B)");
    if ((!vols && !no_volume(cfg)) || !packed || !feat || !h || !c || !rgb_sigma)
        return fail(CNERF_EINVAL, "field_store16: NULL argument (vols, packed, feat, h, c, rgb_sigma)");
    if (counts_of(cfg).n_film && (!freq || !phase)) return fail(CNERF_EINVAL, "field_store16: FiLM layers need freq and phase");
    if (pass != 2 && !cam2world) return fail(CNERF_EINVAL, "field_store16: NULL argument (cam2world of a ray pass)");
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "field_store16: the fine pass needs fine_z");
    if (pass == 2 && !u_strat) return fail(CNERF_EINVAL, "field_store16: pass 2 takes the points (B,R*R*S,3) in the u_strat argument");
    // explicit points need no camera: packed stands in for the address pass_args offsets (it dereferences nothing)
    FieldArgs fa;
    if (int rc = pass_args(fa, cfg, pass, image0, n_images, vols, nullptr, packed, freq, phase, pass == 2 ? packed : cam2world, u_strat, fine_z)) return rc;
    if (pass == 2) fa.cam2world = nullptr;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S;
    return store16_forward(fa, cfg->H, (long long)n_images * npi, feat, h, c, rgb_sigma, (hipStream_t)stream);
}

int cnerf_field_store_pw16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const cnerf_volumes* vols, const float* packed,
                           const float* cam2world, const float* u_strat, const float* fine_z, void* feat, void* h, void* c, float* amax,
                           float* rgb_sigma, void* stream) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;        // (drop_p != 0 with a half-precision cfg is refused here)
    if (cfg->layer_kind[0] != CNERF_LAYER_PFILM)
        return fail(CNERF_EINVAL, "field_store_pw16: per-point FiLM networks only (FiLM / plain-sine / residual layers: cnerf_field_store16)");
    if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "field_store_pw16: single 32-channel volume only");
    if (cfg->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "field_store_pw16: a stage of the fp16 backward: cfg->precision must be CNERF_PREC_FP16X3");
    if (pass < 0 || pass > 2) return fail(CNERF_EINVAL, "field_store_pw16: pass must be 0 (coarse), 1 (fine) or 2 (explicit points)");
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "field_store_pw16: image range out of [0,B)");
    if (!vols || !packed || !feat || !h || !c || !amax || !rgb_sigma)
        return fail(CNERF_EINVAL, "field_store_pw16: NULL argument (vols, packed, feat, h, c, amax, rgb_sigma)");
    if (pass != 2 && !cam2world) return fail(CNERF_EINVAL, "field_store_pw16: NULL argument (cam2world of a ray pass)");
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "field_store_pw16: the fine pass needs fine_z");
    if (pass == 2 && !u_strat) return fail(CNERF_EINVAL, "field_store_pw16: pass 2 takes the points (B,R*R*S,3) in the u_strat argument");
    // explicit points need no camera: packed stands in for the address pass_args offsets (it dereferences nothing)
    FieldArgs fa;
    if (int rc = pass_args(fa, cfg, pass, image0, n_images, vols, nullptr, packed, nullptr, nullptr, pass == 2 ? packed : cam2world, u_strat, fine_z)) return rc;
    if (pass == 2) fa.cam2world = nullptr;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S;
    return store_pw16_forward(fa, cfg->H, (long long)n_images * npi, feat, h, c, amax, rgb_sigma, (hipStream_t)stream);
}

int cnerf_field_chain_pw16(const cnerf_cfg* cfg, int32_t pass, int32_t image0, int32_t n_images, const void* packed16, const float* cam2world,
                           const float* u_strat, const float* fine_z, const float* grad_rgb_sigma, const float* saved_rgb_sigma, const void* cos16,
                           const float* amax, const void* m16, int32_t group_step, void* gy16, void* g16, void* go16, float* scales, uint32_t* gmax,
                           const cnerf_grad_volumes* grad_vols, uint32_t* saturated, void* stream_) {
    g_err[0] = 0;
    if (int rc = check_cfg(cfg, true)) return rc;
    if (cfg->layer_kind[0] != CNERF_LAYER_PFILM)
        return fail(CNERF_EINVAL, "field_chain_pw16: per-point FiLM networks only (FiLM / plain-sine / residual layers: cnerf_field_chain16)");
    if (cfg->C != 32 || cfg->n_levels > 1) return fail(CNERF_EINVAL, "field_chain_pw16: single 32-channel volume only");
    if (cfg->precision != CNERF_PREC_FP16X3) return fail(CNERF_EINVAL, "field_chain_pw16: a stage of the fp16 backward: cfg->precision must be CNERF_PREC_FP16X3");
    if (pass < 0 || pass > 2) return fail(CNERF_EINVAL, "field_chain_pw16: pass must be 0 (coarse), 1 (fine) or 2 (explicit points)");
    if (image0 < 0 || n_images < 1 || image0 + n_images > cfg->B) return fail(CNERF_EINVAL, "field_chain_pw16: image range out of [0,B)");
    if (group_step < 0) return fail(CNERF_EINVAL, "field_chain_pw16: group_step=%d must be 0 (the render's rule) or >= 1", group_step);
    if (!packed16 || !grad_rgb_sigma || !saved_rgb_sigma || !cos16 || !amax || !m16 || !gy16 || !g16 || !go16 || !scales || !gmax || !grad_vols)
        return fail(CNERF_EINVAL,
                    "field_chain_pw16: NULL argument (packed16, grad_rgb_sigma, saved_rgb_sigma, cos16, amax, m16, gy16, g16, go16, scales, gmax, grad_vols)");
    if (int rc = check_grad_vols(cfg, grad_vols, "field_chain_pw16")) return rc;
    if (pass != 2 && !cam2world) return fail(CNERF_EINVAL, "field_chain_pw16: NULL argument (cam2world of a ray pass)");
    if (pass == 1 && !fine_z) return fail(CNERF_EINVAL, "field_chain_pw16: the fine pass needs fine_z");
    if (pass == 2 && !u_strat) return fail(CNERF_EINVAL, "field_chain_pw16: pass 2 takes the points (B,R*R*S,3) in the u_strat argument");
    // the chain reads no volume, no forward weights and (explicit points) no camera: packed16 stands in for the addresses pass_args wants
    // to see (it offsets them and dereferences nothing); they are taken out again below
    const float* stand_in = (const float*)packed16;
    cnerf_volumes unread;
    memset(&unread, 0, sizeof(unread));
    unread.level[0] = stand_in;
    FieldArgs fa;
    if (int rc = pass_args(fa, cfg, pass, image0, n_images, &unread, grad_vols, nullptr, nullptr, nullptr, pass == 2 ? stand_in : cam2world, u_strat, fine_z))
        return rc;
    fa.lvl_vol[0] = nullptr;
    if (pass == 2) fa.cam2world = nullptr;
    hipStream_t stream = (hipStream_t)stream_;
    const long long npi = (long long)cfg->R * cfg->R * cfg->S, tpi = (npi + 31) / 32;
    // only channels 0..3 of a row of the head gradient are ever written: the rest must read as zero (the render zeroes its buffer once per call)
    if (hipError_t e = hipMemsetAsync(go16, 0, (size_t)n_images * tpi * 2048, stream)) return hip_fail(e, "memset");
    return chain_pw16_sequence(cfg, packed16, fa, n_images, npi, tpi, grad_rgb_sigma + (size_t)image0 * npi * 4, saved_rgb_sigma + (size_t)image0 * npi * 4,
                               cos16, amax, m16, gy16, g16, go16, gmax, scales, group_step, saturated, stream);
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

// cnerf_field_query_backward (abi_common.hpp: cnerf_render_rays_backward checks both of its field passes with check_only before its first
// kernel, then runs them)
extern "C++" int cnerf::query_backward(bool check_only, const cnerf_cfg* cfg, int32_t bprec, int64_t points_per_chunk, const cnerf_volumes* vols, const cnerf_field_params* P,
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

}  // extern "C"
