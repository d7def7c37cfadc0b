// Internal interface between the C-ABI translation unit and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/cnerf.h"
#include "cnerf_dev.hpp"

namespace cnerf {

enum { FIELD_MODE_POINTS = 0, FIELD_MODE_COARSE = 1, FIELD_MODE_FINE = 2 };

// Arguments of field_tile_kernel (passed by value).
struct FieldArgs {
    // layer-0 inputs: n_in tiles of 32 channels; in_level[tk] = pyramid level (or -1: the xyz tile), in_chan[tk] = first
    // channel inside that level.  lvl_vol: (B,V,V,V,C) channel-last; lvl_grad: same shape, backward only.
    int n_in;
    int in_level[8];
    int in_chan[8];
    const float* lvl_vol[CNERF_MAX_LEVELS];
    float* lvl_grad[CNERF_MAX_LEVELS];
    int lvl_V[CNERF_MAX_LEVELS];
    int lvl_C[CNERF_MAX_LEVELS];
    const float* packed;     // packed weights (float4 stream, see field_kernel.hip)
    const float* bias;       // biases of all layers then the head, inside the packed buffer
    const float* freq;       // (B, film_stride) or null
    const float* phase;
    const float* points;     // mode POINTS: (B,n,3)
    const float* cam2world;  // (B,16)
    const float* u_strat;    // mode COARSE: (B,n) or null
    const float* fine_z;     // mode FINE: (B,n)
    float* rgb_sigma;        // (B,n,4)
    float* z_out;            // mode COARSE: (B,n)
    float* points_out;       // optional (B,n,3)
    void* unused;            // never read: keeps the argument layout the kernels were tuned in (dropping these 8 bytes moves every later
                             // field off its 16-byte alignment; the compiler then groups the argument loads differently and 18 of the
                             // field kernels change their spills, e.g. the fp32 activation-storing re-run at H = 256 from 0 to 68 bytes)
    // activation store of the backward pass (all null in a plain forward): row-major [point][channel]
    long long act_points;    // rows of every activation buffer (= B * n_per_image of the chunk)
    float* act_feat;         // (n,32*n_in) layer-0 input tiles (looked-up features, xyz)
    float* act_h;            // (L,n,H) layer outputs sin(arg)
    float* act_c;            // (L,n,H) cos(arg)
    int act_tb16;            // 1: act_feat / act_h / act_c are fp16 buffers in the TB16 layout (bwd16.hpp), written by field_h3_kernel
    float* act_amax;         // per-point FiLM family, act_tb16: (L, tiles * 32) largest |stored derivative| per layer and point (field_pw16.hip)
    // field_backward_kernel only
    const float* packed_t;   // transposed packed weights (cnerf_pack_field_transposed)
    const float* grad_out;   // (n,4) d loss / d rgb_sigma
    const float* saved_out;  // (n,4) rgb_sigma of the forward (sigmoid')
    float* act_g;            // (L,n,H) d loss / d arg
    float* act_go;           // (n,4)   d loss / d head pre-activation
    float* gin;              // chain16_kernel, ray passes: (feature input tiles, points of the launch, 32) fp32 gradients of the looked-up features,
                             // scattered by scatter_patch_kernel; null: the chain scatters its tiles itself (explicit points)
    long long n_per_image;
    long long tiles_per_image;
    long long total_tiles;
    RayGeom geom;
    float half_voxel;
    int L;
    int n_mats;              // weight matrices before the head (a residual block counts two)
    int film_stride;
    int bias_floats;         // biases of all layers + head (padded to 4): ones[H], zeros[H] follow
    uint32_t flags;
    int mode;
    int layer_kind[CNERF_MAX_LAYERS];
    PhiloxKey philox;        // in-kernel draw of u_strat where the tensor is null (cnerf_cfg.philox_*)
    int image0;              // first image of this launch inside the call (global element indices of the draws)
    // dropout behind the sine of the FiLM / sine / per-point FiLM layers (training mode, cnerf_cfg.drop_p); drop_scale 0 = off
    float drop_scale;        // 1 / (1 - p)
    uint32_t drop_thresh;    // Philox word >= thresh keeps (thresh = round(p * 2^32))
    uint32_t drop_stream;    // Philox stream of this pass (PHILOX_DROP_*)
    int n_drop;              // dropout layers of the network (= layers that are not residual blocks)
    long long drop_points;   // points of the whole call (B * n_per_image): row count of one layer of drop_mask
    const uint8_t* drop_mask;  // injected keep decisions (n_drop, drop_points, H), 1 = keep; null: Philox
    // folded FiLM constants of the call (field_tile_kernel FOLD: all-FiLM networks, plain fp32 forward), or null
    const float* fold;       // [Mh | Ml | K | Kb], each (fold_images, n_mats, H)
    int fold_images;
    const float* packed_img; // WFOLD: per image, the layer part of the packed weights with rows scaled by Mh (scale_packed_kernel), or null
    long long packed_img_stride;
};

// ---- host side of the kernels that run one block of four waves per CU (the fp16 kernels: 512 registers per wave) ----------------
constexpr size_t LDS_LIMIT = 160 * 1024;         // LDS of a CU: the most a block can ask for

inline int cu_count() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
    return cus;
}

// blocks for the groups of 4 tiles of one image: at most one per CU, a multiple of 8 (every XCD class owns an eighth: group_range())
inline int one_block_per_cu_grid(const FieldArgs& a) {
    const long long want = (a.total_tiles / a.tiles_per_image) * ((a.tiles_per_image + 3) / 4);
    const int cus = cu_count();
    int blocks = (int)(want < cus ? want : cus);
    if (blocks < 8) blocks = 8;
    return (blocks + 7) / 8 * 8;
}

// f: the geometry the grid is sized from (the forward kernels' own argument; the chains carry it inside theirs).  lds_attr_bytes: the
// kernel's dynamic-LDS allowance (>= lds_bytes), set per launch, not once per process: the attribute is per device, and a cached
// flag would be unsynchronised global state
template <typename Args>
inline hipError_t launch_per_cu(void (*kernel)(Args), const FieldArgs& f, size_t lds_bytes, size_t lds_attr_bytes, const Args& args, hipStream_t stream) {
    if (hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_attr_bytes)) return e;
    hipLaunchKernelGGL(kernel, dim3(one_block_per_cu_grid(f)), dim3(256), lds_bytes, stream, args);
    return hipGetLastError();
}

// hidden width -> the kernels' template parameter: f(std::integral_constant<int, NT>{}) with NT = H / 32 output tiles
template <typename F>
inline hipError_t dispatch_nt(int H, F f) {
    switch (H / 32) {
        case 2: return f(std::integral_constant<int, 2>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_fill(float* dst, float value, int n, hipStream_t stream);
hipError_t launch_pack_matrix(const float* w, int n_out, int K_real, int OT, float* dst, hipStream_t stream);
hipError_t launch_fold_film(const FieldArgs& a, int B, int H, float* out, hipStream_t stream);
hipError_t launch_scale_packed(const FieldArgs& a, int B, int H, const float* mh, long long layer_floats, float* out, hipStream_t stream);
hipError_t launch_field(const FieldArgs& a, int H, hipStream_t stream);
hipError_t launch_field_h3(const FieldArgs& a, int H, hipStream_t stream);
hipError_t launch_field_h1(const FieldArgs& a, int H, hipStream_t stream);      // field_h3.hip compiled with CNERF_H3_PARTS=1
// per-image weight folding of the fp16 kernels (field_h3.hip): img (B, img_elems fp16), fold (B, n_mats * (H + 1)), rowf (B, n_mats, H) scratch
hipError_t launch_fold_h3(const FieldArgs& a, int B, int H, void* img, float* fold, float* rowf, long long img_elems, hipStream_t stream);
hipError_t launch_fold_h1(const FieldArgs& a, int B, int H, void* img, float* fold, float* rowf, long long img_elems, hipStream_t stream);
// t_stride: fragment pairs (one per (output tile, k-chunk)) between successive output tiles in dst; 0 = dense
hipError_t launch_pack_h1(const float* w, int n_out, int K_real, int OT, bool k_outer, void* dst, float* inv_scale_slot, float* wmax_slot,
                          hipStream_t stream, long long t_stride = 0);
hipError_t launch_pack_h3(const float* w, int n_out, int K_real, int OT, bool k_outer, void* dst, float* inv_scale_slot, float* wmax_slot,
                          hipStream_t stream, long long t_stride = 0);
// field_pw16.hip (compiled twice like field_h3.hip): the per-point FiLM family (TALLSIREN) on the fp16 matrix pipe
hipError_t launch_field_pw3(const FieldArgs& a, int H, hipStream_t stream);
hipError_t launch_field_pw1(const FieldArgs& a, int H, hipStream_t stream);
// starting values of the accumulators (biases in accumulator units) and the epilogue's scalars from the raw biases and the 1 / S slots
hipError_t launch_pw16_consts(const cnerf_field_params* p, int L, int H, const float* inv_s, float* consts, hipStream_t stream);
hipError_t launch_field_backward(const FieldArgs& a, int H, hipStream_t stream);
hipError_t launch_pack_head_t(const float* w, int H, float* dst, hipStream_t stream);
hipError_t launch_pack_head(const float* w, int H, float* dst, hipStream_t stream);
hipError_t launch_pack_matrix_t(const float* w, int n_rows_w, int n_cols_w, int OT, float* dst, hipStream_t stream);

// ray_kernels.hip
struct CompositeArgs {
    const float* rgb_sigma;  // (rays,n,4)
    const float* z;          // (rays,n)
    const float* eps;        // (rays,n) or null
    float* rgb;              // (rays,3) or null
    float* dist;             // (rays) or null
    float* weights;          // (rays,n) or null
    long long rays;
    int n;
    float noise_std;
    uint32_t flags;
};
hipError_t launch_composite(const CompositeArgs& a, hipStream_t stream);

struct ResampleArgs {
    const float* z;        // (rays,S)
    const float* weights;  // (rays,S) or null when rgb_sigma is given
    const float* rgb_sigma;  // (rays,S,4): if non-null the coarse weights are composited here first
    const float* eps;      // (rays,S) or null
    const float* u;        // (rays,S)
    float* fine_z;         // (rays,S)
    int32_t* inds;         // optional
    float* cdf;            // optional (rays,S-1)
    float* weights_out;    // optional (rays,S)
    long long rays;
    int S;
    float noise_std;
    uint32_t flags;
    PhiloxKey philox;      // draws eps (coarse) / u (fine) in the kernel where the tensors are null
};
hipError_t launch_resample(const ResampleArgs& a, hipStream_t stream);

struct MergeArgs {
    const float* coarse_rgb_sigma;  // (rays,S,4)
    const float* coarse_z;          // (rays,S)
    const float* fine_rgb_sigma;    // (rays,S,4) or null (non-hierarchical)
    const float* fine_z;            // (rays,S)   or null
    const float* eps;               // (rays,n) or null, n = 2S or S
    float* pixels;                  // (B,3,R,R); per_ray: (rays,3)
    float* depth;                   // (B,R,R);   per_ray: (rays) distance along the ray
    int32_t* sort_idx;              // optional (rays,2S)
    float* final_weights;           // optional (rays,n)
    long long rays;
    int S;
    RayGeom geom;
    float noise_std;
    uint32_t flags;
    PhiloxKey philox;               // draws eps (final) in the kernel where the tensor is null
    int per_ray;                    // 1: a ray batch -- outputs per ray, geom is not read (0: the R x R grid's image layout and depth)
};
hipError_t launch_merge_composite(const MergeArgs& a, hipStream_t stream);

struct MergeBwdArgs {
    const float* coarse_rgb_sigma;  // (rays,S,4) saved by the forward
    const float* coarse_z;          // (rays,S)
    const float* fine_rgb_sigma;    // (rays,S,4) or null
    const float* fine_z;            // (rays,S)   or null
    const float* eps;               // (rays,n) or null
    const float* grad_pixels;       // (B,3,R,R); per_ray: (rays,3)
    const float* grad_depth;        // (B,R,R) or null; per_ray: (rays) d loss / d distance
    float* grad_coarse;             // (rays,S,4)
    float* grad_fine;               // (rays,S,4) or null
    long long rays;
    int S;
    RayGeom geom;
    float noise_std;
    uint32_t flags;
    PhiloxKey philox;
    int per_ray;                    // as MergeArgs
};
hipError_t launch_merge_composite_backward(const MergeBwdArgs& a, hipStream_t stream);

// ray_batch.hip: sample positions of caller-given rays, and the rays' gradients from those of the sample positions
struct RaySampleArgs {
    const float* origins;    // (rays,3) world
    const float* dirs;       // (rays,3) world, not normalised here: depths are in units of |dir|
    const float* z;          // (rays,S) depths to sample at, or null: the stratified coarse depths from ...
    const float* u_strat;    // ... (rays,S) jitter draws, or null: Philox stream 0 at the element's index, or 0.5
    float* z_out;            // (rays,S) the coarse depths (z == null only)
    float* points;           // (rays,S,3) o + d z
    long long rays;
    int S;
    float ray_start, ray_end;
    PhiloxKey philox;
    const float* near;       // (rays) per-ray interval of the coarse depths in place of ray_start ...
    const float* far;        // ... and ray_end (z == null only), or both null: the two scalars
};
hipError_t launch_ray_sample(const RaySampleArgs& a, hipStream_t stream);
struct RayGradArgs {         // grad_origins (rays,3) += sum_s g, grad_dirs (rays,3) += sum_s z g (each may be null)
    const float* grad_points;  // (rays,S,3)
    const float* z;            // (rays,S)
    float* grad_origins;
    float* grad_dirs;
    long long rays;
    int S;
};
hipError_t launch_ray_grad_reduce(const RayGradArgs& a, hipStream_t stream);

// occupancy.hip: occupancy bits from corner densities, the stable compaction of the live points of every image, the expansion of their values
struct OccGrid {             // cnerf_occupancy on the device side
    const uint32_t* bits;    // (B, G^3 / 32): bit (ix G + iy) G + iz of an image in word idx >> 5, bit idx & 31
    int G;
    float lo[3];
    float inv;               // (float)G / side, rounded once on the host
};
struct OccBuildArgs {
    const float* sigma;      // (B, (G+1)^3) densities at the cell corners, index (ix (G+1) + iy) (G+1) + iz
    uint32_t* bits;          // (B, G^3 / 32)
    int B, G, dilate;
    float threshold;
};
constexpr int OCC_CHUNK = 2048;      // points of an image one block counts and ranks (8 rounds of 256)
inline long long occ_chunks(long long n) { return (n + OCC_CHUNK - 1) / OCC_CHUNK; }
struct OccCompactArgs {
    OccGrid grid;
    const float* points;     // (B,n,3)
    int32_t* rank;           // (B,n): index among the image's live points in ascending order, -1 = skipped
    float* live_points;      // (B,n,3): the live positions of image b packed at the front of its n rows
    int32_t* counts;         // (B) live points per image
    int32_t* block_counts;   // (B, occ_chunks(n)) scratch: live points per chunk, then their exclusive offsets
    long long n;
    int B;
};
struct OccExpandArgs {
    const int32_t* rank;            // (B,n)
    const float* live_rgb_sigma;    // (B,n,4): image b's values at the front of its n rows
    float* rgb_sigma;               // (B,n,4)
    long long n;
    int B;
};
struct OccBoundsArgs {       // per-ray [near, far] from the grid: include/cnerf.h states the contract
    OccGrid grid;
    float cell;              // side / (float)G, rounded once on the host: plane j of axis k is lo[k] + (float)j * cell
    const float* origins;    // (B,P,3)
    const float* dirs;       // (B,P,3)
    float* near;             // (B,P)
    float* far;              // (B,P)
    uint8_t* hit;            // (B,P) or null
    long long P;
    int B;
    float t_min, t_max, pad;
};
hipError_t launch_occ_build(const OccBuildArgs& a, hipStream_t stream);
hipError_t launch_occ_ray_bounds(const OccBoundsArgs& a, hipStream_t stream);
hipError_t launch_occ_compact(const OccCompactArgs& a, hipStream_t stream);
hipError_t launch_occ_expand(const OccExpandArgs& a, hipStream_t stream);
// rows of `chunks` counts each -> their exclusive offsets in place and the rows' totals in counts (rows): one block per row
hipError_t launch_occ_scan(int32_t* block_counts, int32_t* counts, int rows, int chunks, hipStream_t stream);

// isosurface.hip: marching tetrahedra on a scalar lattice (include/cnerf.h states the algorithm, DESIGN.md 3.19 the workspace)
constexpr int ISO_BLOCK = 256;       // lattice points of a block, one per lane: the unit of the block sums
struct IsoDims {
    int n0, n1, n2;
    int n;                   // n0 n1 n2 <= 2^27
    int blocks;              // ceil(n / ISO_BLOCK)
};
inline IsoDims iso_dims(int n0, int n1, int n2) {
    const int n = n0 * n1 * n2;
    return IsoDims{n0, n1, n2, n, (n + ISO_BLOCK - 1) / ISO_BLOCK};
}
struct IsoCountArgs {
    IsoDims d;
    const float* values;     // (n0,n1,n2)
    float level;
    uint8_t* code;           // (n) INSIDE bits of the point (bit 0) and its seven forward neighbours (bit d0 + 2 d1 + 4 d2)
    int32_t* voff;           // (n) vertices owned by the points before this one in its block
    int32_t* toff;           // (n) triangles of the cells before this one in its block
    int32_t* block_sums;     // (2, blocks) vertices, triangles per block; after the scan their exclusive offsets
    int32_t* counts;         // (2) vertices, triangles
};
struct IsoEmitArgs {
    IsoDims d;
    const float* values;
    float level;
    float lo[3];
    float pitch;
    const float* attrs;      // (n0,n1,n2,n_attr) or null
    int n_attr;              // 0 without attrs
    long long max_vertices, max_triangles;
    float* vertices;         // (max_vertices,3)
    float* vertex_attrs;     // (max_vertices,n_attr) or null
    int32_t* triangles;      // (max_triangles,3)
    const uint8_t* code;
    const int32_t* voff;
    const int32_t* toff;
    const int32_t* block_offsets;    // (2, blocks)
};
hipError_t launch_iso_count(const IsoCountArgs& a, hipStream_t stream);
hipError_t launch_iso_emit(const IsoEmitArgs& a, hipStream_t stream);

// components.hip: connected components of a scalar lattice by a union-find in `labels` (include/cnerf.h states the contract, DESIGN.md 3.25 the protocol)
constexpr int COMP_BLOCK = ISO_BLOCK;        // lattice points of a block, one per lane: IsoDims.blocks counts these
struct CompLabelArgs {
    IsoDims d;
    const float* values;         // (n0,n1,n2)
    float level;
    int invert;                  // 0: the INSIDE points (v > level) are selected, 1: all the others
    int kinds;                   // forward neighbour kinds: 3 (axes: connectivity 6) or 7 (the Kuhn edges: connectivity 14)
    int32_t* labels;             // (n) the parent array, in the end the root (smallest flat index of the component) or -1
    int32_t* sizes;              // (n) points of the component at its root, 0 elsewhere
    int32_t* stats;              // (4) components, root and size of the largest, status
    unsigned long long* best;    // workspace: size << 32 | (0xFFFFFFFF - root) of the largest
};
struct CompFilterArgs {
    IsoDims d;
    const float* values;
    const int32_t* labels;
    const int32_t* sizes;
    const int32_t* stats;
    int largest_only, min_size;
    float fill;
    float* out;                  // (n), may be values
};
hipError_t launch_components_label(const CompLabelArgs& a, hipStream_t stream);
hipError_t launch_components_filter(const CompFilterArgs& a, hipStream_t stream);

// nearest.hip: exact nearest target of every query, brute force (include/cnerf.h states the contract, DESIGN.md 3.20 the tiling)
constexpr int NN_QPT = 4;                    // queries a lane owns in registers
constexpr int NN_QUERIES = NN_QPT * 64;      // queries of a block (one wave): cnerf_nearest_points_tiling's queries_per_block
constexpr int NN_TILE = 16;                  // targets a wave holds in scalar registers at a time: its targets_per_tile
struct NearestArgs {
    int B;
    long long n, m;
    int splits;                // >= 1: ranges the targets of an image are cut into
    const float* queries;      // (B,n,3)
    const float* targets;      // (B,m,3)
    const int32_t* n_queries;  // (B) or null
    const int32_t* n_targets;  // (B) or null
    float* dist2;              // (B,n)
    int32_t* idx;              // (B,n)
    float* part_d;             // (B,splits,n), splits > 1 only
    int32_t* part_j;           // (B,splits,n), splits > 1 only
};
hipError_t launch_nearest_points(const NearestArgs& a, hipStream_t stream);

// voxelize.hip: voxel grids of coloured point clouds and their first-hit pictures (include/cnerf.h states the contracts, DESIGN.md 3.21 the design)
struct VoxelizeArgs {
    int B;
    long long n;               // rows per image, < 2^28
    int stride;                // floats per row, >= 6: xyz rgb first
    const float* points;       // (B,n,stride)
    const int32_t* n_points;   // (B) or null
    int G;
    float lo[3];
    float inv;                 // (float)G / side, rounded once on the host
    int clip;                  // 1: coordinates are clamped into [clip_lo, clip_hi] first and no point is outside
    float clip_lo[3], clip_hi[3];      // lo + m, (lo + side) - m, each operation rounded on the host
    int layout;                // 0: [b, ch, iz, iy, ix]   1: [b, ix, iy, iz, ch]
    float* voxels;
    int32_t* counts;           // (B,G,G,G) in the layout's spatial order, or null
    unsigned long long* acc;   // workspace (B, G^3, 4): count, sum r, sum g, sum b per cell in the layout's cell order
};
struct VoxelHitArgs {
    int B;
    long long P;
    const float* origins;      // (B,P,3)
    const float* dirs;         // (B,P,3)
    const float* voxels;       // a grid per image in `layout`
    int G;
    float lo[3];
    float inv;
    int layout;
    float t_min, t_max;
    int S;
    float background[3];
    float* pixels;             // (B,P,3)
    float* hit_t;              // (B,P) or null
    int32_t* hit_cell;         // (B,P) or null
};
hipError_t launch_voxelize(const VoxelizeArgs& a, hipStream_t stream);
hipError_t launch_voxel_first_hit(const VoxelHitArgs& a, hipStream_t stream);

// reproject.hip: depth maps -> one fused cloud, and the z-buffered picture of a cloud (include/cnerf.h states the contracts, DESIGN.md 3.22 the design)
constexpr int BP_CHUNK = 256;        // pixels of a view one block counts and emits, one per lane
inline int bp_chunks(int R) { return (R * R + BP_CHUNK - 1) / BP_CHUNK; }
struct BackprojectArgs {
    int V, R;
    int chunks;                // bp_chunks(R): blocks per view
    const float* depth;        // (V,R,R)
    const float* colors;       // (V,3,R,R) in layout 0, (V,R,R,3) in layout 1, or null
    int color_layout;
    const float* mask;         // (V,R,R) or null
    const float* cam2world;    // (V,16)
    float focal, z_min, z_max, mask_min, color_scale, color_offset;
    float* points;             // (V R R, out_stride): the valid pixels' rows at the front, in ascending (v, row, col)
    int out_stride;            // 6 with colours, else 3
    int32_t* counts;           // (V) or null
    int32_t* pixel;            // (V R R) or null: (v R + row) R + col of every row of the cloud
    int32_t* rank;             // (V,R,R) or null: the pixel's row in the cloud, -1 = not valid
    int32_t* chunk_counts;     // workspace (V chunks + 1): valid pixels per chunk, then their exclusive offsets and the total
};
struct SplatArgs {
    int B;
    long long n;               // rows per image, < 2^28
    int stride;                // floats per row, >= 3; 6 or more with pixels
    const float* points;       // (B,n,stride)
    const int32_t* n_points;   // (B) or null
    int V, R;
    const float* cam2world;    // (B,V,16)
    float focal, z_min, z_max;
    int radius;
    float background[3];
    float* depth;              // (B,V,R,R) or null
    int32_t* index;            // (B,V,R,R) or null
    float* pixels;             // (B,V,R,R,3) or null
    unsigned long long* keys;  // workspace (B,V,R,R): bits(z) << 32 | point index of the nearest point so far
};
hipError_t launch_backproject(const BackprojectArgs& a, hipStream_t stream);
hipError_t launch_splat_points(const SplatArgs& a, hipStream_t stream);

// tsdf.hip: V depth maps -> a truncated signed distance lattice (include/cnerf.h states the contract, DESIGN.md 3.23 the design)
struct TsdfArgs {
    int n0, n1, n2;            // lattice, axis c = world axis c; n0 n1 n2 <= 2^27
    float lo[3], pitch;        // point i sits at (float)i_c * pitch + lo[c]
    int V, R;
    const float* depth;        // (V,R,R)
    const float* colors;       // (V,3,R,R) in layout 0, (V,R,R,3) in layout 1, or null
    int color_layout;
    float color_scale, color_offset;
    const float* cam2world;    // (V,16)
    float focal, z_min, z_max, trunc;
    int carve;                 // 1: a background pixel is an observation of -1
    int hidden_min;            // > 0: a voxel no view saw free and this many saw behind a surface is 1
    float unseen;
    float* tsdf;               // (n0,n1,n2)
    int32_t* weight;           // (n0,n1,n2) or null
    float* rgb;                // (n0,n1,n2,3) or null
};
hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t stream);

hipError_t launch_philox_fill(const PhiloxKey& k, uint32_t stream_id, long long n, int normal, float* out, hipStream_t stream);
hipError_t launch_transpose_cl(int B, int C, int V, const float* src, float* dst, bool to_channel_last, hipStream_t stream);

struct GatherArgs {
    const float* fvol;    // (B,V,V,V,C)
    const float* points;  // (B,n,3)
    float* feat;          // (B,n,C)
    long long n_per_image;
    int B, V, C;
    float half_voxel;
};
hipError_t launch_gather(const GatherArgs& a, hipStream_t stream);
// scatter_patch.hip: feature-volume gradient of a ray pass from the chain's stored input-tile gradients, pre-reduced per pixel patch x depth bin in LDS
hipError_t launch_scatter_patch(const FieldArgs& f, const float* gin, hipStream_t stream);
hipError_t launch_scatter(const GatherArgs& a, const float* grad_feat, float* grad_fvol, hipStream_t stream);

// points_grad.hip: the position gradient of a field query (never launched by the render path)
struct InputGradArgs {       // out (n, ldo)[:, 0:k_in) = (g (.) f) W * inv_scale
    const float* g32;        // fp32 rows (n, ldg), or null: ...
    const void* g16;         // ... a TB16 fp16 slab with g_ct channel tiles (chunk-local tiles: point p is row p % 32 of tile p / 32)
    long long ldg;
    int g_ct;
    const float* inv_scale;  // device scalar undoing the slab's scale, or null
    const float* f;          // (K) factor per row of W (FiLM frequencies of the layer), or null
    const float* W;          // (K, k_in) row-major
    int K, k_in;             // K a multiple of 32
    float* out;
    long long ldo;
    long long n;
};
struct PointsGradArgs {      // grad_points (n,3) += lookup term of gfeat + gxyz
    const float* lvl_vol[CNERF_MAX_LEVELS];  // one image's channel-last levels
    int lvl_V[CNERF_MAX_LEVELS];
    int lvl_C[CNERF_MAX_LEVELS];
    int n_levels;
    const float* points;     // (n,3)
    const float* gfeat;      // (n, ldf): the levels' channels side by side
    long long ldf;
    const float* gxyz;       // (n, ldx) d loss / d xyz of layer 0's input, or null
    long long ldx;
    float* grad_points;      // (n,3) accumulated into
    long long n;
    float half_voxel;
};
hipError_t launch_input_grad(const InputGradArgs& a, hipStream_t stream);
hipError_t launch_points_lookup_grad(const PointsGradArgs& a, hipStream_t stream);
hipError_t launch_drop_keep(const PhiloxKey& k, uint32_t stream_id, uint32_t thresh, int n_drop, int H, unsigned long long gp0,
                            long long n_points, uint8_t* mask, hipStream_t stream);

hipError_t launch_weight_grad(int cnt, long long npi, int H, int K, const float* G, const float* X, float* dW, float* colsum,
                              hipStream_t stream);
hipError_t launch_param_reduce(int cnt, int rows, int ld, int k_real, const float* dWarg, const float* cs, const float* freq, int film_stride,
                               const float* W, const float* bias, float* dW, float* db, float* g_freq, float* g_phase, hipStream_t stream);
hipError_t launch_head_grad32(const float* go, const float* x, long long n, int H, float* dW, float* db, hipStream_t stream);
hipError_t launch_absmax_bits(const float* v, long long n, uint32_t* slot, hipStream_t stream);
hipError_t launch_pow2_scales(const uint32_t* gmax_bits, int n, float* scales, hipStream_t stream);

// pfilm_finish.hip: mapping-network stage of the per-point FiLM family's exact fp32 backward (cnerf_pfilm_backward_finish)
hipError_t launch_pack_pfilm_map(const float* wm1, const float* wm2, int K2, float* dst, hipStream_t stream);
hipError_t launch_pfilm_gm32(const float* packed_map, const float* G, const float* m, long long n, int K2, float* g_mpre, float* d_feat,
                             hipStream_t stream);
hipError_t launch_layer0_grad32(const float* g, const float* pts, long long n, int H, float* dW, float* db, hipStream_t stream);

// bwd16.hip
hipError_t launch_pack_t16(const float* w, int n_rows_w, int n_cols_w, int n_cols_real, int OT_padded, void* dst, float* winv_slot, uint32_t* wmax_slot,
                           hipStream_t stream);
hipError_t launch_col_abs_sum_max(const float* w, int n_rows, int n_cols, float* slot, hipStream_t stream);
hipError_t launch_pack_head_t16(const float* w, int H, void* dst, float* winv_slot, uint32_t* wmax_slot, hipStream_t stream);
hipError_t launch_chain16(const FieldArgs& f, int H, const void* units, const void* head_t, const float* winv, const float* scales, const void* cos16,
                          void* g16, void* go16, unsigned int* gmax, unsigned int* sat, int nslab, int dry, int group_step, hipStream_t stream);
hipError_t launch_weight_grad16(int cnt, long long tiles_per_image, int n_rows, int g_ct, int x_ct, const void* G, const void* X, float* dW,
                                float* colsum, const float* inv_scale, hipStream_t stream);

// chain_pw16.hip: half-precision gradient chain of the per-point FiLM family (chain_pre_kernel + pw_gm_kernel)
struct PwChainBuffers {
    const void* units_y;      // Y units: W_l^T, stages L-2 .. 0 (launch_pack_pw_chain)
    const void* units_m;      // M units: the Wm2 pair of every layer by channel tile, then Wm1^T
    const void* head_t;
    const float* winv;        // [W_l^T: L (0 unused) | Wm2 pair of layer l: L | Wm1^T | head^T]
    const float* anorm;       // [||W_l||_1: L (0 unused) | head]
    const float* scales;      // {S, 1 / S} x (4 L + 2): per layer (g_pre, g_fr, g_ph), g_mpre, go, then g_y per layer
    const float* lay;         // per layer {r_l, To_l} (launch_pw_split_scales)
    const void* cos16;        // 3 L COS16 slabs of the storing forward
    const float* amax;        // (L, tiles * 32)
    const void* m16;          // TB16 (tiles, 8, 32, 32)
    void* gy16;               // TB16: L slabs (tiles, NT, 32, 32) of g_y
    void* g16;                // TB16: 3 L slabs (tiles, NT, 32, 32) then g_mpre (tiles, 8, 32, 32)
    void* go16;
    unsigned int* gmax;       // dry runs: 3 L: g_mpre, 3 L + 1: go, 3 L + 2 + l: g_y of layer l
    unsigned int* sat;
};
hipError_t launch_chain_pre(const FieldArgs& f, int H, const PwChainBuffers& c, int dry, int group_step, hipStream_t stream);
hipError_t launch_pw_gm(const FieldArgs& f, int H, const PwChainBuffers& c, int dry, int group_step, hipStream_t stream);
hipError_t launch_pw_split_scales(const uint32_t* amaxg_bits, int L, float* scales, float* lay, hipStream_t stream);
size_t pw_chain_y_bytes(int L, int H);
size_t pw_chain_m_bytes(int L, int H);
hipError_t launch_pack_pw_chain(const cnerf_field_params* p, int L, int H, void* units_y, void* units_m, void* head_t, float* winv, float* anorm,
                                uint32_t* wmax, hipStream_t stream);

}  // namespace cnerf
