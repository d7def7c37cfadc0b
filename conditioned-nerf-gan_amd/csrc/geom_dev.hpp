// Rules that two or more of the geometry kernels share, each stated once in the order include/cnerf.h words it, every operation rounded
// on its own.  Device code, but for capped_grid at the end.
#pragma once
#include "cnerf_dev.hpp"

namespace cnerf {

// World point p -> pixel of the pinhole camera M (cam2world, 16 floats row-major), in two steps: a caller rejects on the depth between them.
__device__ __forceinline__ float cam_depth(const float* M, const float* p, float (&q)[3]) {       // q = p - t; returns q . third column
    q[0] = __fsub_rn(p[0], M[3]), q[1] = __fsub_rn(p[1], M[7]), q[2] = __fsub_rn(p[2], M[11]);
    return __fadd_rn(__fadd_rn(__fmul_rn(q[0], M[2]), __fmul_rn(q[1], M[6])), __fmul_rn(q[2], M[10]));
}
// u = ((cx f) / z) half + half, v from cy, half = 0.5 (R - 1).  Callers compare them as floats (a NaN fails, what passes converts), then rintf.
__device__ __forceinline__ void cam_pixel(const float (&q)[3], float z, const float* M, float focal, float half, float& u, float& v) {
    const float cx = __fadd_rn(__fadd_rn(__fmul_rn(q[0], M[0]), __fmul_rn(q[1], M[4])), __fmul_rn(q[2], M[8]));
    const float cy = __fadd_rn(__fadd_rn(__fmul_rn(q[0], M[1]), __fmul_rn(q[1], M[5])), __fmul_rn(q[2], M[9]));
    u = __fadd_rn(__fmul_rn(__fmul_rn(cx, focal) / z, half), half);
    v = __fadd_rn(__fmul_rn(__fmul_rn(cy, focal) / z, half), half);
}

// Lattices: point i of an axis sits at (float)i * pitch + lo, the product rounded, then the sum; the flat index is (i0 n1 + i1) n2 + i2.
__device__ __forceinline__ float lattice_pos(int i, float pitch, float lo) { return __fadd_rn(__fmul_rn((float)i, pitch), lo); }
struct Index3 { int i0, i1, i2; };
__device__ __forceinline__ Index3 lattice_split(int e, int n1, int n2) {
    const int i2 = e % n2, q = e / n2, i1 = q % n1;
    return Index3{q / n1, i1, i2};
}

// Cells of a cube: t = (p - lo) * inv on an axis, inside iff 0 <= t < G (a NaN is not inside), and then the cell is floorf(t).
__device__ __forceinline__ float cell_coord(float p, float lo, float inv) { return __fmul_rn(__fsub_rn(p, lo), inv); }
__device__ __forceinline__ bool cell_inside(float t, float Gf) { return t >= 0.0f && t < Gf; }

// Rows of image b that count: lens[b] clamped into [0, full]; all of them without lens.  (b in the caller's own integer type.)
template <typename Int>
__device__ __forceinline__ long long clamped_len(const int32_t* __restrict__ lens, Int b, long long full) {
    if (!lens) return full;
    const long long v = lens[b];
    return v < 0 ? 0 : (v > full ? full : v);
}

// Colours of pixel pix of view v, (V,3,R,R) in layout 0 and (V,R,R,3) in layout 1: channel 0 and the step between channels; c * scale + offset.
struct ViewColor { const float* c; size_t step; };
__device__ __forceinline__ ViewColor view_color_at(const float* colors, int layout, size_t v, size_t RR, size_t pix) {
    return ViewColor{layout == 0 ? colors + v * 3 * RR + pix : colors + (v * RR + pix) * 3, layout == 0 ? RR : 1};
}
__device__ __forceinline__ float view_color(const ViewColor& at, int ch, float scale, float offset) {
    return __fadd_rn(__fmul_rn(at.c[ch * at.step], scale), offset);
}

// Stable compaction in a block of WAVES waves, without atomics: live lanes before this one in the block, and the block's live lanes.
struct BlockRank { int before, total; };
// One count per wave -> the waves before and the block: LDS, one barrier.  `slot` (WAVES ints) is the caller's: no reuse while a slow wave reads.
template <int WAVES>
__device__ __forceinline__ BlockRank block_wave_sums(int wave_count, int* slot) {
    const int wave = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) slot[wave] = wave_count;
    __syncthreads();
    BlockRank r{0, 0};
    for (int w = 0; w < WAVES; ++w) r.before += w < wave ? slot[w] : 0, r.total += slot[w];
    return r;
}
template <int WAVES>
__device__ __forceinline__ BlockRank block_rank(bool live, int* slot) {      // ballot + popcount per wave: lanes below and waves before
    const unsigned long long mask = __ballot(live);
    BlockRank r = block_wave_sums<WAVES>(__popcll(mask), slot);
    r.before += __popcll(mask & ((1ull << (threadIdx.x & (WAVE - 1))) - 1ull));
    return r;
}

// Host: blocks of a launch whose kernel strides over what is beyond `cap`; at least 1, though every caller's checks rule out an empty launch.
inline unsigned capped_grid(long long blocks, long long cap) { return (unsigned)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap)); }

}  // namespace cnerf
