// Between a depth image and world-space points: cnerf_backproject lifts the valid pixels of V depth maps into one fused cloud (a stable
// compaction), cnerf_splat_points pictures a cloud from cameras with a z-buffer.  include/cnerf.h states both contracts (arithmetic, the
// validity rule, the key), DESIGN.md section 3.22 the design, tests/reproject_common.py restates them in NumPy.
//
// Replaces the host code of the reference's Inferencer.render_pcl (inference.py:541-559: nonzero, indexing and a 4x4 matmul on the CPU,
// in a Python loop over the views) and gives what its render_pcl_masked / loss_depth read from EXR files: a depth image of the cloud.
//
// back-projection   count, scan, emit over the flat pixel sequence (v, row, col), as occupancy.hip compacts sample points: a block owns
//   count            BP_CHUNK = 256 consecutive pixels of one view (one round, one pixel per lane); geom_dev.hpp's block_rank gives the
//                    block's total.  chunk_counts (V, chunks per view): the flat pixel order.
//   scan             occupancy.hip's occ_scan_kernel over the V * chunks counts as ONE row: exclusive offsets in place, the total behind
//                    them.  No atomics anywhere: the order of the cloud is the pixels' own.
//   emit             the validity again, the pixel's row from the chunk's offset and block_rank's lanes before; the twelve separately
//                    rounded operations of the position, the colour (view_color), rank, pixel; block 0 of a view writes counts[v] as a
//                    difference of two offsets.
// splat             the workspace is one 64-bit key per (b, view, row, col), set to all ones.
//   splat            one lane per (point, view); a block handles one (b, view) and 256 points, so the camera and the scalars are
//                    wave-uniform.  Key = bits(z) << 32 | point index; z is a positive finite float, whose bits order like its value.
//                    One no-return 64-bit unsigned atomic min at agent scope per covered pixel (behind a plain load iff radius > 0).
//                    A minimum does not depend on the order of arrival: the result is the same bits for every launch geometry and run.
//   resolve          one lane per pixel: the key back into depth, index and the winner's stored colour.
// The two splat kernels stride over their work with a grid of at most SPLAT_MAX_GRID blocks.  The projection is geom_dev.hpp's.
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int RP_BLOCK = 256;                      // threads of every block here: four waves; BP_CHUNK (cnerf_kernels.hpp) is the same number
constexpr int RP_WAVES = RP_BLOCK / WAVE;
constexpr long long SPLAT_MAX_GRID = 2048;         // blocks of a splat launch (8 per CU); the kernels stride over what is beyond
static_assert(BP_CHUNK == RP_BLOCK, "a block counts and emits one pixel per lane");

#ifndef CNERF_SPLAT_EARLY_OUT
#define CNERF_SPLAT_EARLY_OUT 1                    // 0: never load the key before the atomic (the A/B build of profiles/reproject.md)
#endif

// ---- back-projection ------------------------------------------------------------------------------------------------------------
// z_min < z < z_max (a NaN is not valid), and mask > mask_min where there is a mask
__device__ __forceinline__ bool bp_valid(const BackprojectArgs& a, long long e, float& z) {
    z = a.depth[e];
    bool ok = a.z_min < z && z < a.z_max;
    if (ok && a.mask) ok = a.mask[e] > a.mask_min;
    return ok;
}

__global__ __launch_bounds__(RP_BLOCK) void bp_count_kernel(BackprojectArgs a) {
    __shared__ int wave_sum[RP_WAVES];
    const int RR = a.R * a.R;
    const int v = blockIdx.x / a.chunks, c = blockIdx.x - v * a.chunks;      // block-uniform
    const int p = c * BP_CHUNK + threadIdx.x;
    float z;
    const bool live = p < RR && bp_valid(a, (long long)v * RR + p, z);
    const int total = block_rank<RP_WAVES>(live, wave_sum).total;
    if (threadIdx.x == 0) a.chunk_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(RP_BLOCK) void bp_emit_kernel(BackprojectArgs a) {
    __shared__ int wave_cnt[RP_WAVES];
    const int RR = a.R * a.R;
    const int v = blockIdx.x / a.chunks, c = blockIdx.x - v * a.chunks;
    const int p = c * BP_CHUNK + threadIdx.x;
    const long long e = (long long)v * RR + p;
    const int total_chunks = a.V * a.chunks;
    float z = 0.0f;
    const bool live = p < RR && bp_valid(a, e, z);
    const int before = block_rank<RP_WAVES>(live, wave_cnt).before;
    const int base = a.chunk_counts[blockIdx.x];
    if (c == 0 && threadIdx.x == 0 && a.counts)          // offsets are flat over the views: a view's count is a difference of two
        a.counts[v] = a.chunk_counts[v + 1 < a.V ? (v + 1) * a.chunks : total_chunks] - base;
    if (p >= RR) return;
    const int k = live ? base + before : -1;
    if (a.rank) a.rank[e] = k;
    if (!live) return;
    if (a.pixel) a.pixel[k] = (int32_t)e;
    const int row = p / a.R, col = p - row * a.R;
    const float Rm1 = (float)(a.R - 1);
    const float xn = (float)(2 * col - (a.R - 1)) / Rm1, yn = (float)(2 * row - (a.R - 1)) / Rm1;
    const float xc = __fmul_rn(xn / a.focal, z), yc = __fmul_rn(yn / a.focal, z);
    const float* M = a.cam2world + (size_t)v * 16;
    float* out = a.points + (size_t)k * a.out_stride;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        out[i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4 * i], xc), __fmul_rn(M[4 * i + 1], yc)), __fmul_rn(M[4 * i + 2], z)), M[4 * i + 3]);
    if (a.colors) {
        const ViewColor cv = view_color_at(a.colors, a.color_layout, v, RR, p);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[3 + ch] = view_color(cv, ch, a.color_scale, a.color_offset);
    }
}

hipError_t launch_backproject(const BackprojectArgs& a, hipStream_t stream) {
    const int blocks = a.V * a.chunks;
    hipLaunchKernelGGL(bp_count_kernel, dim3(blocks), dim3(RP_BLOCK), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = launch_occ_scan(a.chunk_counts, a.chunk_counts + blocks, 1, blocks, stream)) return e;
    hipLaunchKernelGGL(bp_emit_kernel, dim3(blocks), dim3(RP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// ---- z-buffered splat -----------------------------------------------------------------------------------------------------------
// look: a plain load of the key first, which skips the atomic that cannot lower it.  Keys only fall, so a stale read can cause an
// unnecessary atomic, never a wrong skip.  Measured (profiles/reproject.md): with footprints (radius > 0) tens of points share a pixel
// and the load saves up to 1.8x; at radius 0 most atomics do lower the key and the load only adds its latency (0.55x at 100,000
// points).  So the kernel looks first iff radius > 0 -- wave-uniform.
__device__ __forceinline__ void splat_min(unsigned long long* p, unsigned long long key, bool look) {
#if CNERF_SPLAT_EARLY_OUT
    if (look && __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
#endif
    __hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}

__global__ __launch_bounds__(RP_BLOCK) void splat_kernel(SplatArgs a) {
    const long long chunks = (a.n + RP_BLOCK - 1) / RP_BLOCK;
    const long long items = (long long)a.B * a.V * chunks;
    const int R = a.R, rad = a.radius;
    const float half = __fmul_rn(0.5f, (float)(R - 1));
    const float lo = -(float)(rad + 1), hi = (float)(R + rad);
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {       // w, and with it b, view and the camera, is block-uniform
        const long long bv = w / chunks;
        const long long i = (w - bv * chunks) * RP_BLOCK + threadIdx.x;
        const long long b = bv / a.V;
        if (i >= clamped_len(a.n_points, b, a.n)) continue;
        const float* M = a.cam2world + (size_t)bv * 16;
        const float* p = a.points + ((size_t)b * a.n + i) * a.stride;
        float q[3], u, v;
        const float z = cam_depth(M, p, q);
        if (!(a.z_min < z && z < a.z_max)) continue;                  // behind, beyond, a NaN
        cam_pixel(q, z, M, a.focal, half, u, v);
        if (!(lo < u && u < hi && lo < v && v < hi)) continue;
        const int col = (int)rintf(u), row = (int)rintf(v);
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (uint32_t)i;
        unsigned long long* img = a.keys + (size_t)bv * R * R;
        const int r0 = max(row - rad, 0), r1 = min(row + rad, R - 1), c0 = max(col - rad, 0), c1 = min(col + rad, R - 1);
        for (int rr = r0; rr <= r1; ++rr)
            for (int cc = c0; cc <= c1; ++cc) splat_min(img + (size_t)rr * R + cc, key, rad > 0);
    }
}

__global__ __launch_bounds__(RP_BLOCK) void splat_resolve_kernel(SplatArgs a) {
    const long long per_b = (long long)a.V * a.R * a.R;
    const long long total = (long long)a.B * per_b;
    for (long long e = (long long)blockIdx.x * RP_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * RP_BLOCK) {
        const unsigned long long key = a.keys[e];
        const bool hit = key != ~0ull;
        const int32_t i = hit ? (int32_t)(uint32_t)key : -1;
        if (a.depth) a.depth[e] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (a.index) a.index[e] = i;
        if (a.pixels) {
            float c0 = a.background[0], c1 = a.background[1], c2 = a.background[2];
            if (hit) {
                const float* p = a.points + ((size_t)(e / per_b) * a.n + i) * a.stride;
                c0 = p[3], c1 = p[4], c2 = p[5];
            }
            float* o = a.pixels + (size_t)e * 3;
            o[0] = c0, o[1] = c1, o[2] = c2;
        }
    }
}

hipError_t launch_splat_points(const SplatArgs& a, hipStream_t stream) {
    const long long px = (long long)a.B * a.V * a.R * a.R;
    if (hipError_t e = hipMemsetAsync(a.keys, 0xff, (size_t)px * sizeof(unsigned long long), stream)) return e;
    const long long chunks = (a.n + RP_BLOCK - 1) / RP_BLOCK;
    hipLaunchKernelGGL(splat_kernel, dim3(capped_grid((long long)a.B * a.V * chunks, SPLAT_MAX_GRID)), dim3(RP_BLOCK), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(splat_resolve_kernel, dim3(capped_grid((px + RP_BLOCK - 1) / RP_BLOCK, SPLAT_MAX_GRID)), dim3(RP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cnerf
