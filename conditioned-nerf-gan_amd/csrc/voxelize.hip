// Voxel grids of coloured point clouds (cnerf_voxelize) and their first-hit pictures (cnerf_voxel_first_hit).  include/cnerf.h states both
// contracts (arithmetic, skips, layouts); DESIGN.md section 3.21 the design and why the colours are summed in fixed point;
// tests/voxelize_common.py restates them in NumPy.
//
// Replaces the reference's offline feature_volume/pcl2voxel.py (open3d's VoxelGrid plus a Python loop over its voxels, one file per
// resolution) and the march of feature_volume/voxel2img.py (grid_sample over every sample of every ray, then a Python loop over the hits).
//
// voxelize    The workspace holds four 64-bit integers per cell -- count, sum r, sum g, sum b -- in the cell order of the OUTPUT layout.
//   clear        hipMemsetAsync.
//   accumulate   one lane per point.  A block's 256 rows come through LDS: the six used columns of the rows are loaded as 6 x 256
//                consecutive dwords (all of the rows when stride = 6), then a lane reads its own row from LDS (rows padded to 7 dwords:
//                an odd pitch, no bank conflict).  Four no-return integer
//                atomics at agent scope into the cell's 32 bytes.  Integer sums do not depend on the order of arrival: the result is the
//                same bits for every launch geometry and every run.
//   finish       one lane per cell: 32 bytes in, the four values out -- coalesced on both sides in either layout.
// first hit   one lane per ray walks the S depths in ascending order and leaves at the first occupied sample.  Per step one fma for the
//             depth (linspace_at, as ATen), then twelve separately rounded operations for the position and the cell coordinate (never
//             fused), one 4-byte load.  No atomics.
// The cell rule and the clamped row count of an image are geom_dev.hpp's.
// Every kernel strides over its work with a grid of at most VOX_MAX_GRID blocks; the tests cross that size in all three.
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int VOX_BLOCK = 256;
constexpr int VOX_PITCH = 7;                     // dwords of a staged row in LDS: six used, odd so that the lanes' reads hit distinct banks
constexpr long long VOX_MAX_GRID = 2048;         // blocks of a launch (8 per CU: every wave slot); the kernels stride over what is beyond
constexpr float VOX_Q = 16777216.0f;             // 2^24: colours are summed as integers in units of 2^-24

__device__ __forceinline__ void vox_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}

// q of the contract: a NaN counts as 0
__device__ __forceinline__ unsigned long long vox_quant(float c) {
    c = c == c ? c : 0.0f;
    return (unsigned long long)(uint32_t)rintf(__fmul_rn(fminf(fmaxf(c, 0.0f), 1.0f), VOX_Q));
}

// cell index per axis, or -1: the point is skipped
__device__ __forceinline__ int vox_axis(const VoxelizeArgs& a, int k, float p) {
    const float Gf = (float)a.G;
    if (a.clip) {
        p = fminf(fmaxf(p, a.clip_lo[k]), a.clip_hi[k]);
        const int i = (int)floorf(cell_coord(p, a.lo[k], a.inv));
        return i < 0 ? 0 : (i > a.G - 1 ? a.G - 1 : i);
    }
    const float t = cell_coord(p, a.lo[k], a.inv);
    if (!cell_inside(t, Gf)) return -1;             // outside, an infinity, an overflow
    return (int)floorf(t);
}

__global__ __launch_bounds__(VOX_BLOCK) void voxelize_accumulate_kernel(VoxelizeArgs a) {
    __shared__ float rows[VOX_BLOCK * VOX_PITCH];
    const long long chunks = (a.n + VOX_BLOCK - 1) / VOX_BLOCK;
    const long long items = (long long)a.B * chunks;
    const long long cells = (long long)a.G * a.G * a.G;
    const int tid = threadIdx.x;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const long long b = w / chunks;
        const long long p0 = (w - b * chunks) * VOX_BLOCK;
        const long long np = clamped_len(a.n_points, b, a.n);
        if (p0 >= np) continue;                      // block-uniform
        const float* src = a.points + ((size_t)b * a.n + p0) * a.stride;
        const long long live = np - p0 < VOX_BLOCK ? np - p0 : VOX_BLOCK;
        __syncthreads();                             // the previous item's rows have been read
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int e = k * VOX_BLOCK + tid;
            const int row = e / 6, col = e - row * 6;
            if (row < live) rows[row * VOX_PITCH + col] = src[(size_t)row * a.stride + col];
        }
        __syncthreads();
        if (tid >= live) continue;
        const float* mine = rows + tid * VOX_PITCH;
        const float x = mine[0], y = mine[1], z = mine[2];
        if (x != x || y != y || z != z) continue;
        const int ix = vox_axis(a, 0, x), iy = vox_axis(a, 1, y), iz = vox_axis(a, 2, z);
        if ((ix | iy | iz) < 0) continue;
        const long long cell = a.layout == 0 ? ((long long)iz * a.G + iy) * a.G + ix : ((long long)ix * a.G + iy) * a.G + iz;
        unsigned long long* acc = a.acc + ((size_t)b * cells + cell) * 4;
        vox_add(acc, 1ull);
        vox_add(acc + 1, vox_quant(mine[3]));
        vox_add(acc + 2, vox_quant(mine[4]));
        vox_add(acc + 3, vox_quant(mine[5]));
    }
}

__global__ __launch_bounds__(VOX_BLOCK) void voxelize_finish_kernel(VoxelizeArgs a) {
    const long long cells = (long long)a.G * a.G * a.G;
    const long long total = (long long)a.B * cells;
    for (long long e = (long long)blockIdx.x * VOX_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * VOX_BLOCK) {
        const ulonglong2* acc = reinterpret_cast<const ulonglong2*>(a.acc + (size_t)e * 4);
        const ulonglong2 cr = acc[0], gb = acc[1];
        const unsigned long long cnt = cr.x;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cnt) {
            const double den = (double)cnt * 16777216.0;
            v[0] = 1.0f;
            v[1] = (float)((double)cr.y / den);
            v[2] = (float)((double)gb.x / den);
            v[3] = (float)((double)gb.y / den);
        }
        if (a.layout == 0) {
            const long long b = e / cells, cell = e - b * cells;
            float* o = a.voxels + (size_t)b * 4 * cells + cell;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) o[(size_t)ch * cells] = v[ch];
        } else {
            reinterpret_cast<float4*>(a.voxels)[e] = make_float4(v[0], v[1], v[2], v[3]);
        }
        if (a.counts) a.counts[e] = (int32_t)cnt;
    }
}

__global__ __launch_bounds__(VOX_BLOCK) void voxel_first_hit_kernel(VoxelHitArgs a) {
    const long long total = (long long)a.B * a.P;
    const long long cells = (long long)a.G * a.G * a.G;
    const float Gf = (float)a.G;
    for (long long r = (long long)blockIdx.x * VOX_BLOCK + threadIdx.x; r < total; r += (long long)gridDim.x * VOX_BLOCK) {
        const long long b = r / a.P;
        const float* vox = a.voxels + (size_t)b * 4 * cells;
        const float ox = a.origins[r * 3], oy = a.origins[r * 3 + 1], oz = a.origins[r * 3 + 2];
        const float dx = a.dirs[r * 3], dy = a.dirs[r * 3 + 1], dz = a.dirs[r * 3 + 2];
        float px0 = a.background[0], px1 = a.background[1], px2 = a.background[2];
        float ht = INFINITY;
        int hc = -1;
        for (int s = 0; s < a.S; ++s) {
            const float t = linspace_at(a.t_min, a.t_max, a.S, s);
            const float tx = cell_coord(__fadd_rn(ox, __fmul_rn(dx, t)), a.lo[0], a.inv);
            const float ty = cell_coord(__fadd_rn(oy, __fmul_rn(dy, t)), a.lo[1], a.inv);
            const float tz = cell_coord(__fadd_rn(oz, __fmul_rn(dz, t)), a.lo[2], a.inv);
            if (!(tx >= 0.0f && tx < Gf && ty >= 0.0f && ty < Gf && tz >= 0.0f && tz < Gf)) continue;      // cell_inside on the three axes, as one chain
            const int ix = (int)floorf(tx), iy = (int)floorf(ty), iz = (int)floorf(tz);
            const long long at = a.layout == 0 ? ((long long)iz * a.G + iy) * a.G + ix : (((long long)ix * a.G + iy) * a.G + iz) * 4;
            const long long ch = a.layout == 0 ? cells : 1;
            if (vox[at] != 0.0f) {                   // a NaN is occupied
                px0 = vox[at + ch], px1 = vox[at + 2 * ch], px2 = vox[at + 3 * ch];
                ht = t;
                hc = (ix * a.G + iy) * a.G + iz;
                break;
            }
        }
        a.pixels[r * 3] = px0, a.pixels[r * 3 + 1] = px1, a.pixels[r * 3 + 2] = px2;
        if (a.hit_t) a.hit_t[r] = ht;
        if (a.hit_cell) a.hit_cell[r] = hc;
    }
}

hipError_t launch_voxelize(const VoxelizeArgs& a, hipStream_t stream) {
    const long long cells = (long long)a.G * a.G * a.G;
    if (hipError_t e = hipMemsetAsync(a.acc, 0, (size_t)a.B * cells * 4 * sizeof(unsigned long long), stream)) return e;
    const long long chunks = (a.n + VOX_BLOCK - 1) / VOX_BLOCK;
    hipLaunchKernelGGL(voxelize_accumulate_kernel, dim3(capped_grid((long long)a.B * chunks, VOX_MAX_GRID)), dim3(VOX_BLOCK), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(voxelize_finish_kernel, dim3(capped_grid(((long long)a.B * cells + VOX_BLOCK - 1) / VOX_BLOCK, VOX_MAX_GRID)), dim3(VOX_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_voxel_first_hit(const VoxelHitArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(voxel_first_hit_kernel, dim3(capped_grid(((long long)a.B * a.P + VOX_BLOCK - 1) / VOX_BLOCK, VOX_MAX_GRID)), dim3(VOX_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cnerf
