// C ABI (include/cnerf.h), shapes: isosurface meshes, lattice components, nearest points, voxel grids of point clouds, depth maps <-> clouds, depth maps -> a TSDF lattice.
#include "abi_common.hpp"

using namespace cnerf;

// checks that more than one entry makes: the message of each is written here alone
namespace {
int check_finite3(const float* v, const char* name, const char* who) {
    for (int c = 0; c < 3; ++c)
        if (!(fabsf(v[c]) < INFINITY)) return fail(CNERF_EINVAL, "%s: %s[%d]=%g must be finite", who, name, c, (double)v[c]);
    return CNERF_OK;
}
int check_pitch(float p, const char* who) { return p > 0.0f && p < INFINITY ? CNERF_OK : fail(CNERF_EINVAL, "%s: pitch=%g must be > 0 and finite", who, (double)p); }
int check_color_layout(int l, const char* who) { return l == 0 || l == 1 ? CNERF_OK : fail(CNERF_EINVAL, "%s: color_layout=%d must be 0 (V,3,R,R) or 1 (V,R,R,3)", who, l); }
int check_cloud_rows(long long n, int stride, int min_stride, const char* who) {
    if (n < 1 || n >= (1LL << 28)) return fail(CNERF_EINVAL, "%s: n=%lld out of range [1,2^28)", who, n);
    if (stride < min_stride) return fail(CNERF_EINVAL, "%s: stride=%d must be >= %d (%s)", who, stride, min_stride, min_stride == 3 ? "xyz" : "xyz rgb");
    return CNERF_OK;
}
}  // namespace

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
    Carver w;
    W.code = w.take((size_t)d.n);
    W.voff = w.take((size_t)d.n * sizeof(int32_t));
    W.toff = w.take((size_t)d.n * sizeof(int32_t));
    W.sums = w.take((size_t)2 * d.blocks * sizeof(int32_t));
    W.total = w.off;
    return W;
}
}  // namespace

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

// ---------------------------------------------------------------------------------------------------------------------
// voxel grids of coloured point clouds and their first-hit pictures (csrc/voxelize.hip)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
int check_voxel_grid(int B, int G, const char* who) {
    if (B < 1) return fail(CNERF_EINVAL, "%s: B=%d must be >= 1", who, B);
    if (G < 2 || G > 256) return fail(CNERF_EINVAL, "%s: G=%d out of range [2,256]", who, G);
    return CNERF_OK;
}
int check_voxel_cube(int G, const float* lo, float side, int layout, const char* who) {
    if (!lo) return fail(CNERF_EINVAL, "%s: lo is NULL", who);
    if (!(side > 0.0f) || !(side < INFINITY)) return fail(CNERF_EINVAL, "%s: side=%g must be > 0 and finite", who, (double)side);
    if (!((float)G / side < INFINITY))       // a denormal side: every cell coordinate would be an infinity or a NaN
        return fail(CNERF_EINVAL, "%s: side=%g is too small: (float)G / side is not finite", who, (double)side);
    if (int rc = check_finite3(lo, "lo", who)) return rc;
    if (layout != 0 && layout != 1) return fail(CNERF_EINVAL, "%s: layout=%d must be 0 (B,4,G,G,G) or 1 (B,G,G,G,4)", who, layout);
    return CNERF_OK;
}
// four 64-bit integers per cell
size_t voxelize_bytes(int B, int G) { return align256((size_t)B * G * G * G * 4 * sizeof(unsigned long long)); }
}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// depth maps <-> clouds: back-projection and the z-buffered splat (csrc/reproject.hip)
// ---------------------------------------------------------------------------------------------------------------------
namespace {
// views (per image: B = 1 for the back-projection) of R x R pixels
int check_view_grid(int B, int V, int R, const char* who) {
    if (B < 1) return fail(CNERF_EINVAL, "%s: B=%d must be >= 1", who, B);
    if (V < 1) return fail(CNERF_EINVAL, "%s: V=%d must be >= 1", who, V);
    if (R < 2 || R > 2048) return fail(CNERF_EINVAL, "%s: R=%d out of range [2,2048]", who, R);
    if ((long long)V * R * R >= (1LL << 31) / B) return fail(CNERF_EINVAL, "%s: B V R R = %d x %d x %d x %d must be below 2^31", who, B, V, R, R);
    return CNERF_OK;
}
int check_pinhole(float focal, float z_min, float z_max, const char* who) {
    if (!(focal > 0.0f) || !(focal < INFINITY)) return fail(CNERF_EINVAL, "%s: focal=%g must be > 0 and finite", who, (double)focal);
    if (!(z_min >= 0.0f) || !(z_min < INFINITY)) return fail(CNERF_EINVAL, "%s: z_min=%g must be >= 0 and finite", who, (double)z_min);
    if (!(z_max > z_min) || !(z_max < INFINITY)) return fail(CNERF_EINVAL, "%s: z_max=%g must be finite and greater than z_min=%g", who, (double)z_max, (double)z_min);
    return CNERF_OK;
}
// the chunk counts of every view, then the total
size_t backproject_bytes(int V, int R) { return align256(((size_t)V * bp_chunks(R) + 1) * sizeof(int32_t)); }
// one 64-bit key per pixel
size_t splat_bytes(int B, int V, int R) { return align256((size_t)B * V * R * R * sizeof(unsigned long long)); }
}  // namespace

extern "C" {

int cnerf_backproject_bytes(int32_t V, int32_t R, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_view_grid(1, V, R, "backproject_bytes")) return rc;
    if (workspace) *workspace = backproject_bytes(V, R);
    return CNERF_OK;
}

int cnerf_backproject(int32_t V, int32_t R, const float* depth, const float* colors, int32_t color_layout, const float* mask, float mask_min,
                      const float* cam2world, float focal, float z_min, float z_max, float color_scale, float color_offset, float* points,
                      int32_t* counts, int32_t* pixel, int32_t* rank, void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "backproject";
    if (int rc = check_view_grid(1, V, R, who)) return rc;
    if (int rc = check_pinhole(focal, z_min, z_max, who)) return rc;
    if (mask_min != mask_min) return fail(CNERF_EINVAL, "%s: mask_min is NaN", who);
    if (color_scale != color_scale || color_offset != color_offset) return fail(CNERF_EINVAL, "%s: color_scale / color_offset is NaN", who);
    if (int rc = check_color_layout(color_layout, who)) return rc;
    if (!depth || !cam2world || !points || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument (depth / cam2world / points / workspace)", who);
    BackprojectArgs a{};
    a.V = V, a.R = R, a.chunks = bp_chunks(R), a.depth = depth, a.colors = colors, a.color_layout = color_layout, a.mask = mask, a.cam2world = cam2world;
    a.focal = focal, a.z_min = z_min, a.z_max = z_max, a.mask_min = mask_min, a.color_scale = color_scale, a.color_offset = color_offset;
    a.points = points, a.out_stride = colors ? 6 : 3, a.counts = counts, a.pixel = pixel, a.rank = rank, a.chunk_counts = (int32_t*)workspace;
    if (hipError_t e = launch_backproject(a, (hipStream_t)stream)) return hip_fail(e, "backproject");
    return CNERF_OK;
}

int cnerf_splat_points_bytes(int32_t B, int32_t V, int32_t R, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_view_grid(B, V, R, "splat_points_bytes")) return rc;
    if (workspace) *workspace = splat_bytes(B, V, R);
    return CNERF_OK;
}

int cnerf_splat_points(int32_t B, int64_t n, int32_t stride, const float* points, const int32_t* n_points, int32_t V, const float* cam2world, int32_t R,
                       float focal, float z_min, float z_max, int32_t radius, const float background[3], float* depth, int32_t* index, float* pixels,
                       void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "splat_points";
    if (int rc = check_view_grid(B, V, R, who)) return rc;
    if (int rc = check_cloud_rows((long long)n, stride, 3, who)) return rc;
    if (pixels && stride < 6) return fail(CNERF_EINVAL, "%s: pixels need stride >= 6 (xyz rgb), got stride=%d", who, stride);
    if (radius < 0 || radius > 8) return fail(CNERF_EINVAL, "%s: radius=%d out of range [0,8]", who, radius);
    if (int rc = check_pinhole(focal, z_min, z_max, who)) return rc;
    if (!points || !cam2world || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument (points / cam2world / workspace)", who);
    if (pixels && !background) return fail(CNERF_EINVAL, "%s: background is NULL and pixels are asked for", who);
    if ((uintptr_t)workspace & 7) return fail(CNERF_EINVAL, "%s: workspace must be 8-byte aligned", who);
    SplatArgs a{};
    a.B = B, a.n = (long long)n, a.stride = stride, a.points = points, a.n_points = n_points, a.V = V, a.R = R, a.cam2world = cam2world;
    a.focal = focal, a.z_min = z_min, a.z_max = z_max, a.radius = radius;
    for (int c = 0; c < 3; ++c) a.background[c] = background ? background[c] : 0.0f;
    a.depth = depth, a.index = index, a.pixels = pixels, a.keys = (unsigned long long*)workspace;
    if (hipError_t e = launch_splat_points(a, (hipStream_t)stream)) return hip_fail(e, "splat_points");
    return CNERF_OK;
}

int cnerf_tsdf_integrate(int32_t n0, int32_t n1, int32_t n2, const float lo[3], float pitch, int32_t V, int32_t R, const float* depth, const float* colors,
                         int32_t color_layout, float color_scale, float color_offset, const float* cam2world, float focal, float z_min, float z_max,
                         float trunc, int32_t carve, int32_t hidden_min, float unseen, float* tsdf, int32_t* weight, float* rgb, void* stream) {
    g_err[0] = 0;
    const char* who = "tsdf_integrate";
    if (int rc = check_iso_shape(n0, n1, n2, who)) return rc;
    if (int rc = check_view_grid(1, V, R, who)) return rc;
    if (!lo || !depth || !cam2world || !tsdf) return fail(CNERF_EINVAL, "%s: NULL argument (lo / depth / cam2world / tsdf)", who);
    if (int rc = check_pitch(pitch, who)) return rc;
    if (int rc = check_finite3(lo, "lo", who)) return rc;
    if (!(trunc > 0.0f) || !(trunc < INFINITY)) return fail(CNERF_EINVAL, "%s: trunc=%g must be > 0 and finite", who, (double)trunc);
    if (int rc = check_pinhole(focal, z_min, z_max, who)) return rc;
    if (!(fabsf(unseen) < INFINITY)) return fail(CNERF_EINVAL, "%s: unseen=%g must be finite", who, (double)unseen);
    if (!(fabsf(color_scale) < INFINITY)) return fail(CNERF_EINVAL, "%s: color_scale=%g must be finite", who, (double)color_scale);
    if (!(fabsf(color_offset) < INFINITY)) return fail(CNERF_EINVAL, "%s: color_offset=%g must be finite", who, (double)color_offset);
    if (int rc = check_color_layout(color_layout, who)) return rc;
    if (carve != 0 && carve != 1) return fail(CNERF_EINVAL, "%s: carve=%d must be 0 or 1", who, carve);
    if (hidden_min < 0) return fail(CNERF_EINVAL, "%s: hidden_min=%d must be >= 0", who, hidden_min);
    if (rgb && !colors) return fail(CNERF_EINVAL, "%s: rgb is asked for and colors is NULL", who);
    TsdfArgs a{};
    a.n0 = n0, a.n1 = n1, a.n2 = n2, a.pitch = pitch, a.V = V, a.R = R, a.depth = depth, a.colors = colors, a.color_layout = color_layout;
    for (int c = 0; c < 3; ++c) a.lo[c] = lo[c];
    a.color_scale = color_scale, a.color_offset = color_offset, a.cam2world = cam2world, a.focal = focal, a.z_min = z_min, a.z_max = z_max, a.trunc = trunc;
    a.carve = carve, a.hidden_min = hidden_min, a.unseen = unseen, a.tsdf = tsdf, a.weight = weight, a.rgb = rgb;
    if (hipError_t e = launch_tsdf_integrate(a, (hipStream_t)stream)) return hip_fail(e, "tsdf_integrate");
    return CNERF_OK;
}

int cnerf_voxelize_bytes(int32_t B, int32_t G, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_voxel_grid(B, G, "voxelize_bytes")) return rc;
    if (workspace) *workspace = voxelize_bytes(B, G);
    return CNERF_OK;
}

int cnerf_voxelize(int32_t B, int64_t n, int32_t stride, const float* points, const int32_t* n_points, int32_t G, const float lo[3], float side,
                   float clip_margin, int32_t layout, float* voxels, int32_t* counts, void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "voxelize";
    if (int rc = check_voxel_grid(B, G, who)) return rc;
    if (int rc = check_cloud_rows((long long)n, stride, 6, who)) return rc;
    if (int rc = check_voxel_cube(G, lo, side, layout, who)) return rc;
    if (clip_margin != clip_margin) return fail(CNERF_EINVAL, "%s: clip_margin is NaN (>= 0 clips, < 0 does not)", who);
    if (clip_margin >= 0.0f && !(2.0f * clip_margin < side))
        return fail(CNERF_EINVAL, "%s: clip_margin=%g leaves nothing of side=%g (2 clip_margin must be < side)", who, (double)clip_margin, (double)side);
    if (!points || !voxels || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument (points / voxels / workspace)", who);
    if (((uintptr_t)workspace & 15) || (layout == 1 && ((uintptr_t)voxels & 15)))
        return fail(CNERF_EINVAL, "%s: workspace (and voxels in layout 1) must be 16-byte aligned", who);
    VoxelizeArgs a{};
    a.B = B, a.n = (long long)n, a.stride = stride, a.points = points, a.n_points = n_points, a.G = G;
    a.inv = (float)G / side;
    a.clip = clip_margin >= 0.0f;
    for (int c = 0; c < 3; ++c) {
        a.lo[c] = lo[c];
        const float hi = lo[c] + side;
        a.clip_lo[c] = a.clip ? lo[c] + clip_margin : 0.0f;
        a.clip_hi[c] = a.clip ? hi - clip_margin : 0.0f;
    }
    a.layout = layout, a.voxels = voxels, a.counts = counts, a.acc = (unsigned long long*)workspace;
    if (hipError_t e = launch_voxelize(a, (hipStream_t)stream)) return hip_fail(e, "voxelize");
    return CNERF_OK;
}

int cnerf_voxel_first_hit(int32_t B, int64_t rays_per_image, const cnerf_rays* rays, const float* voxels, int32_t G, const float lo[3], float side,
                          int32_t layout, float t_min, float t_max, int32_t S, const float background[3], float* pixels, float* hit_t, int32_t* hit_cell,
                          void* stream) {
    g_err[0] = 0;
    const char* who = "voxel_first_hit";
    if (int rc = check_voxel_grid(B, G, who)) return rc;
    if (rays_per_image < 1 || rays_per_image > (1LL << 38) / B)
        return fail(CNERF_EINVAL, "%s: rays_per_image=%lld must be >= 1 (and B * rays_per_image <= 2^38)", who, (long long)rays_per_image);
    if (int rc = check_voxel_cube(G, lo, side, layout, who)) return rc;
    if (S < 2 || S > 1024) return fail(CNERF_EINVAL, "%s: S=%d out of range [2,1024]", who, S);
    if (!(fabsf(t_min) < INFINITY) || !(fabsf(t_max) < INFINITY)) return fail(CNERF_EINVAL, "%s: t_min=%g and t_max=%g must be finite", who, (double)t_min, (double)t_max);
    if (!(t_min < t_max)) return fail(CNERF_EINVAL, "%s: t_max=%g must be greater than t_min=%g", who, (double)t_max, (double)t_min);
    if (!rays || !rays->origins || !rays->dirs) return fail(CNERF_EINVAL, "%s: NULL argument (rays / rays.origins / rays.dirs)", who);
    if (!voxels || !background || !pixels) return fail(CNERF_EINVAL, "%s: NULL argument (voxels / background / pixels)", who);
    VoxelHitArgs a{};
    a.B = B, a.P = (long long)rays_per_image, a.origins = rays->origins, a.dirs = rays->dirs, a.voxels = voxels, a.G = G;
    a.inv = (float)G / side;
    for (int c = 0; c < 3; ++c) a.lo[c] = lo[c], a.background[c] = background[c];
    a.layout = layout, a.t_min = t_min, a.t_max = t_max, a.S = S, a.pixels = pixels, a.hit_t = hit_t, a.hit_cell = hit_cell;
    if (hipError_t e = launch_voxel_first_hit(a, (hipStream_t)stream)) return hip_fail(e, "voxel_first_hit");
    return CNERF_OK;
}

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
    if (int rc = check_pitch(pitch, who)) return rc;
    if (int rc = check_finite3(lo, "lo", who)) return rc;
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

// connected components of a lattice (csrc/components.hip).  The refusals come in one order: shape, NULLs, level, connectivity, the
// switches, min_size, fill.  Workspace: the 64-bit key of the largest component.
int cnerf_components_bytes(int32_t n0, int32_t n1, int32_t n2, size_t* workspace) {
    g_err[0] = 0;
    if (int rc = check_iso_shape(n0, n1, n2, "components_bytes")) return rc;
    if (workspace) *workspace = align256(sizeof(unsigned long long));
    return CNERF_OK;
}

int cnerf_components_label(int32_t n0, int32_t n1, int32_t n2, const float* values, float level, int32_t invert, int32_t connectivity, int32_t* labels,
                           int32_t* sizes, int32_t* stats, void* workspace, void* stream) {
    g_err[0] = 0;
    const char* who = "components_label";
    if (int rc = check_iso_shape(n0, n1, n2, who)) return rc;
    if (!values || !labels || !sizes || !stats || !workspace) return fail(CNERF_EINVAL, "%s: NULL argument (values / labels / sizes / stats / workspace)", who);
    if (!(fabsf(level) < INFINITY)) return fail(CNERF_EINVAL, "%s: level=%g must be finite", who, (double)level);
    if (connectivity != 6 && connectivity != 14) return fail(CNERF_EINVAL, "%s: connectivity=%d must be 6 or 14", who, connectivity);
    if (invert != 0 && invert != 1) return fail(CNERF_EINVAL, "%s: invert=%d must be 0 or 1", who, invert);
    if ((uintptr_t)workspace & 7) return fail(CNERF_EINVAL, "%s: workspace must be 8-byte aligned", who);
    const CompLabelArgs a{iso_dims(n0, n1, n2), values, level, invert, connectivity == 6 ? 3 : 7, labels, sizes, stats, (unsigned long long*)workspace};
    if (hipError_t e = launch_components_label(a, (hipStream_t)stream)) return hip_fail(e, "components_label");
    return CNERF_OK;
}

int cnerf_components_filter(int32_t n0, int32_t n1, int32_t n2, const float* values, const int32_t* labels, const int32_t* sizes, const int32_t* stats,
                            int32_t largest_only, int32_t min_size, float fill, float* out_values, void* stream) {
    g_err[0] = 0;
    const char* who = "components_filter";
    if (int rc = check_iso_shape(n0, n1, n2, who)) return rc;
    if (!values || !labels || !sizes || !stats || !out_values) return fail(CNERF_EINVAL, "%s: NULL argument (values / labels / sizes / stats / out_values)", who);
    if (largest_only != 0 && largest_only != 1) return fail(CNERF_EINVAL, "%s: largest_only=%d must be 0 or 1", who, largest_only);
    if (min_size < 0) return fail(CNERF_EINVAL, "%s: min_size=%d must be >= 0", who, min_size);
    if (fill != fill) return fail(CNERF_EINVAL, "%s: fill is NaN", who);
    const CompFilterArgs a{iso_dims(n0, n1, n2), values, labels, sizes, stats, largest_only, min_size, fill, out_values};
    if (hipError_t e = launch_components_filter(a, (hipStream_t)stream)) return hip_fail(e, "components_filter");
    return CNERF_OK;
}

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
