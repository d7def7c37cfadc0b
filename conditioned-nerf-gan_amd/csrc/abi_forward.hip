// C ABI (include/cnerf.h), forward side: version and error text, Philox fills, workspace sizes, volume transposes, weight packing, the
// forward stages and cnerf_render_forward on the R x R grid.
#include "abi_common.hpp"

using namespace cnerf;

namespace {
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
    Carver w;
    F.c_rs = w.take(N * 4 * sizeof(float));
    F.f_rs = w.take(N * 4 * sizeof(float));
    F.c_z = w.take(N * sizeof(float));
    F.f_z = w.take(N * sizeof(float));
    if (c->precision != CNERF_PREC_FP32 && c->layer_kind[0] != CNERF_LAYER_PFILM) {
        F.img16 = w.take(B * pl.weight_floats * sizeof(float));
        F.fold16 = w.take(B * mats * (H + 1) * sizeof(float));
        F.rowf = w.take(B * mats * H * sizeof(float));
    } else {
        F.layer_floats = (long long)((NT * nc.n_in + (mats - 1) * NT * NT) * 1024);
        F.fold = w.take(4 * B * mats * H * sizeof(float));
        F.packed_img = w.take(B * (size_t)F.layer_floats * sizeof(float));
    }
    F.total = w.off;
    return F;
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
    if (int rc = check_render("render_forward", cfg, cam2world != nullptr, vols, packed, freq, phase, pixels, depth, workspace, rng)) return rc;
    const bool hier = cfg->flags & CNERF_F_HIERARCHICAL;
    hipStream_t stream = (hipStream_t)stream_;

    const long long P = (long long)cfg->R * cfg->R, npi = P * cfg->S;
    const ForwardLayout F = forward_layout(cfg);
    char* ws = (char*)workspace;

    FieldArgs fa;
    if (int rc = fill_field_args(fa, cfg, vols, nullptr, packed, freq, phase)) return rc;
    set_points(fa, cfg->B, npi);
    fa.cam2world = cam2world;
    // the half-precision activations a training forward keeps for the backward (aux->act16)
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
    // one field pass: the fused kernel samples the grid's rays itself, in coarse or fine mode
    auto field_pass = [&](bool fine, const RenderBuffers& b) -> int {
        fa.mode = fine ? FIELD_MODE_FINE : FIELD_MODE_COARSE;
        fa.u_strat = fine ? nullptr : rng->u_strat;
        fa.fine_z = fine ? b.f_z : nullptr;
        fa.rgb_sigma = fine ? b.f_rs : b.c_rs;
        fa.z_out = fine ? nullptr : b.c_z;
        fa.points_out = fine ? b.f_pts : b.c_pts;
        const auto* act = keep ? &aux->act16[fine] : nullptr;
        fa.act_points = (long long)cfg->B * npi;
        fa.act_feat = keep ? (float*)act->feat : nullptr;
        fa.act_h = keep ? (float*)act->h : nullptr;
        fa.act_c = keep ? (float*)act->c : nullptr;
        fa.act_amax = keep ? (float*)act->amax : nullptr;
        fa.act_tb16 = keep ? 1 : 0;
        set_dropout(fa, cfg, fine ? rng->drop_fine : rng->drop_coarse, fine ? PHILOX_DROP_FINE : PHILOX_DROP_COARSE, npi);
        auto mark = [&](int i) { if (aux && aux->field_events[i]) (void)hipEventRecord((hipEvent_t)aux->field_events[i], stream); };
        mark(2 * fine);
        if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, fine ? "field kernel (fine)" : "field kernel (coarse)");
        mark(2 * fine + 1);
        return CNERF_OK;
    };
    const RenderBuffers b{(float*)(ws + F.c_rs), (float*)(ws + F.f_rs), (float*)(ws + F.c_z), (float*)(ws + F.f_z), nullptr, nullptr};
    return render_sequence(cfg, (long long)cfg->B * P, rng, aux, b, make_geom(cfg), 0, pixels, depth, field_pass, stream);
}

}  // extern "C"
