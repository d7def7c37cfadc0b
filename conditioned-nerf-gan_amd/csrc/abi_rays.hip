// C ABI (include/cnerf.h), rays: renders of caller-given ray batches, forward and backward, per-ray sampling bounds, occupancy grids and
// the renders they mask.
#include "abi_common.hpp"

using namespace cnerf;

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
    Carver w;
    F.c_rs = w.take(N * 4 * sizeof(float));
    F.f_rs = w.take(N * 4 * sizeof(float));
    F.c_z = w.take(N * sizeof(float));
    F.f_z = w.take(N * sizeof(float));
    F.pts = w.take(N * 3 * sizeof(float));
    F.total = w.off;
    return F;
}
// Workspace of cnerf_render_rays_backward: d loss / d rgb_sigma of the coarse and fine samples (N, 4), the positions of the pass in flight
// and their gradients (N, 3 each), then the workspace of a field query of P S points per image
struct RaysBackwardLayout {
    size_t gc, gf, pts, gpts, query, total;
};
int rays_backward_layout(const cnerf_cfg* c, int bprec, long long P, long long ppc, RaysBackwardLayout& R) {
    size_t query_bytes;
    if (int rc = cnerf_field_query_backward_workspace_bytes(c, bprec, ppc, &query_bytes)) return rc;
    const size_t N = (size_t)c->B * (size_t)P * c->S;
    Carver w;
    R.gc = w.take(N * 4 * sizeof(float));
    R.gf = w.take((c->flags & CNERF_F_HIERARCHICAL) ? N * 4 * sizeof(float) : 0);
    R.pts = w.take(N * 3 * sizeof(float));
    R.gpts = w.take(N * 3 * sizeof(float));
    R.query = w.take(query_bytes);
    R.total = w.off;
    return CNERF_OK;
}

// occupancy grids (the masked renders below)
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
    Carver w{M.F.total};
    M.live_pts = w.take(N * 3 * sizeof(float));
    M.live_rs = w.take(N * 4 * sizeof(float));
    M.rank = w.take(N * sizeof(int32_t));
    M.counts = w.take((size_t)c->B * sizeof(int32_t));
    M.compact = w.take(occ_compact_bytes(c->B, P * c->S));
    M.total = w.off;
    return M;
}
}  // namespace

// The render sequence on ray batches: a pass samples its depths and positions (ray_sample), then field(fine, points, rgb_sigma) runs
// the network on them -- all that the plain and the masked render differ in.  F: the forward pieces of the workspace `ws`.
template <class Field>
static int render_rays_sequence(const cnerf_cfg* cfg, const cnerf_rays* rays, long long P, const float* near, const float* far, const cnerf_rng* rng,
                                float* pixels, float* dist, const cnerf_aux* aux, char* ws, const RaysForwardLayout& F, Field&& field, hipStream_t stream) {
    const long long n_rays = (long long)cfg->B * P;
    float* pts = (float*)(ws + F.pts);
    const RenderBuffers bufs{(float*)(ws + F.c_rs), (float*)(ws + F.f_rs), (float*)(ws + F.c_z), (float*)(ws + F.f_z), pts, pts};
    auto field_pass = [&](bool fine, const RenderBuffers& b) -> int {
        // coarse: stratified depths and their positions; fine: the positions at the resampled depths
        float* points = fine ? b.f_pts : b.c_pts;
        const RaySampleArgs sa{rays->origins, rays->dirs, fine ? b.f_z : nullptr, fine ? nullptr : rng->u_strat, fine ? nullptr : b.c_z, points, n_rays,
                               cfg->S, cfg->ray_start, cfg->ray_end, philox_of(cfg), near, far};
        if (hipError_t e = launch_ray_sample(sa, stream)) return hip_fail(e, fine ? "ray_sample (fine)" : "ray_sample (coarse)");
        return field(fine, points, fine ? b.f_rs : b.c_rs);
    };
    // outputs per ray
    return render_sequence(cfg, n_rays, rng, aux, bufs, RayGeom{}, 1, pixels, dist, field_pass, stream);
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
    if (int rc = check_render(who, cfg, true, vols, packed, freq, phase, pixels, dist, workspace, rng)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    // both field passes: the network at explicit points, no dropout (refused above)
    FieldArgs fa;
    if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, nullptr, 0, cfg->B, P * cfg->S, nullptr)) return rc;
    auto field = [&](bool fine, const float* pts, float* rs) -> int {
        fa.points = pts;
        fa.rgb_sigma = rs;
        if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, fine ? "field kernel (fine)" : "field kernel (coarse)");
        return CNERF_OK;
    };
    return render_rays_sequence(cfg, rays, P, near, far, rng, pixels, dist, aux, (char*)workspace, rays_forward_layout(cfg, P), field, stream);
}

extern "C" {

int cnerf_render_rays_workspace_bytes(const cnerf_cfg* cfg, int64_t rays_per_image, size_t* fwd_ws) {
    g_err[0] = 0;
    if (int rc = check_rays_cfg(cfg, (long long)rays_per_image, "render_rays_workspace_bytes")) return rc;
    if (fwd_ws) *fwd_ws = rays_forward_layout(cfg, (long long)rays_per_image).total;
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

// ---------------------------------------------------------------------------------------------------------------------
// occupancy grids: forward-only ray renders that skip empty space (csrc/occupancy.hip)
// ---------------------------------------------------------------------------------------------------------------------

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
    const int B = cfg->B;
    const long long npi = P * cfg->S;
    if (int rc = check_occ_points(B, npi, who)) return rc;
    if (int rc = check_render(who, cfg, true, vols, packed, freq, phase, pixels, dist, workspace, rng)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    // the live counts come back to the host between the compaction and the field launches: not something a graph can record
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipError_t e = hipStreamIsCapturing(stream, &capturing)) return hip_fail(e, "hipStreamIsCapturing");
    if (capturing != hipStreamCaptureStatusNone)
        return fail(CNERF_EINVAL, "%s: the stream is being captured; this call copies the live counts to the host and synchronises", who);

    const MaskedLayout M = masked_layout(cfg, P);
    char* ws = (char*)workspace;
    float* live_pts = (float*)(ws + M.live_pts);
    float* live_rs = (float*)(ws + M.live_rs);
    int32_t* rank = (int32_t*)(ws + M.rank);
    int32_t* counts = (int32_t*)(ws + M.counts);
    // every refusal of the field passes before the first launch (the arguments of image 0 stand for all)
    FieldArgs fa;
    if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, live_pts, 0, 1, npi, nullptr)) return rc;
    int32_t* own_counts = live_counts ? nullptr : (int32_t*)malloc((size_t)B * sizeof(int32_t));
    if (!live_counts && !own_counts) return fail(CNERF_EINVAL, "%s: out of host memory", who);

    // the field on the live points of `pts`: compact, counts to the host (live_counts: coarse then fine), the field per image, expand into rs
    auto field = [&](bool fine, const float* pts, float* rs) -> int {
        int32_t* host_counts = live_counts ? live_counts + (fine ? B : 0) : own_counts;
        const OccCompactArgs ca{grid, pts, rank, live_pts, counts, (int32_t*)(ws + M.compact), npi, B};
        if (hipError_t e = launch_occ_compact(ca, stream)) return hip_fail(e, "occ_compact");
        if (hipError_t e = hipMemcpyAsync(host_counts, counts, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, stream)) return hip_fail(e, "live counts");
        if (hipError_t e = hipStreamSynchronize(stream)) return hip_fail(e, "live counts");
        for (int b = 0; b < B; ++b) {
            if (host_counts[b] <= 0) continue;
            if (int rc = points_args(fa, cfg, vols, nullptr, packed, freq, phase, live_pts + (size_t)b * npi * 3, b, 1, host_counts[b], nullptr)) return rc;
            fa.rgb_sigma = live_rs + (size_t)b * npi * 4;
            if (hipError_t e = launch_forward(fa, cfg, stream)) return hip_fail(e, fine ? "field kernel (fine)" : "field kernel (coarse)");
        }
        if (hipError_t e = launch_occ_expand(OccExpandArgs{rank, live_rs, rs, npi, B}, stream)) return hip_fail(e, "occ_expand");
        return CNERF_OK;
    };
    const int rc = render_rays_sequence(cfg, rays, P, near, far, rng, pixels, dist, aux, ws, M.F, field, stream);
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
