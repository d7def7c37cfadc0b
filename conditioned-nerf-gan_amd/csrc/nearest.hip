// Nearest points (cnerf_nearest_points): for every query of a batched cloud the nearest target of the same image, exactly, by brute
// force.  include/cnerf.h states the contract (arithmetic, tie rule, non-finite values); DESIGN.md section 3.20 the tiling and why it is
// brute force; tests/nearest_common.py restates it in NumPy.
//
// search   One wave per block.  A lane owns NN_QPT queries in registers, as NN_QPT / 2 two-wide vectors so that the three differences,
//          three products and two sums of a pair of queries are packed fp32 operations (each half rounds as the scalar operation does;
//          the build contracts nothing into an fma).  A target is the same address for every lane, so it comes through the scalar data
//          path: the wave walks its range of targets in tiles of NN_TILE, a tile is NN_TILE * 3 consecutive floats in scalar registers,
//          and every vector operation takes the target's component as its scalar operand.  No LDS, no barrier, no atomics.
//          Targets are scanned in ascending order with a strict <, from best = +inf: the lowest index among equal distances wins, and a
//          distance that is NaN or +inf never compares below the best, so it is never chosen.
//          A work item is (image, range of targets, group of NN_QUERIES queries); blocks stride over the items, so no grid dimension
//          grows with the problem beyond NN_MAX_GRID.  With one range the result goes to the outputs, otherwise to the workspace.
//          The clamped lengths of an image (clamped_len) and the capped launch grid are geom_dev.hpp's.
// reduce   (more than one range) one lane per query: the ranges' partial (d, j) in ascending range order under the same strict <.
//          A range holds ascending indices and the ranges ascend, so this is the order of a single scan.
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

typedef float nn_f32x2 __attribute__((ext_vector_type(2)));

constexpr int NN_PAIRS = NN_QPT / 2;
constexpr int NN_REDUCE_BLOCK = 256;
constexpr long long NN_MAX_GRID = 1LL << 20;     // blocks of a launch; the kernels stride over what is beyond
static_assert(NN_QPT % 2 == 0 && NN_QUERIES == NN_QPT * WAVE, "a lane owns whole pairs of queries, a block is one wave");

// one target against the lane's queries; j ascends from call to call
__device__ __forceinline__ void nn_step(const nn_f32x2 (&qx)[NN_PAIRS], const nn_f32x2 (&qy)[NN_PAIRS], const nn_f32x2 (&qz)[NN_PAIRS], float tx, float ty,
                                        float tz, int j, float (&best)[NN_QPT], int (&bj)[NN_QPT]) {
#pragma unroll
    for (int p = 0; p < NN_PAIRS; ++p) {
        const nn_f32x2 dx = qx[p] - tx, dy = qy[p] - ty, dz = qz[p] - tz;
        const nn_f32x2 d = (dx * dx + dy * dy) + dz * dz;
        if (d.x < best[2 * p]) {
            best[2 * p] = d.x;
            bj[2 * p] = j;
        }
        if (d.y < best[2 * p + 1]) {
            best[2 * p + 1] = d.y;
            bj[2 * p + 1] = j;
        }
    }
}

__global__ __launch_bounds__(WAVE) void nearest_search_kernel(int B, long long n, long long m, int splits, const float* __restrict__ queries,
                                                              const float* __restrict__ targets, const int32_t* __restrict__ n_queries,
                                                              const int32_t* __restrict__ n_targets, float* __restrict__ out_d,
                                                              int32_t* __restrict__ out_j) {
    const long long qgroups = (n + NN_QUERIES - 1) / NN_QUERIES;
    const long long items = (long long)B * splits * qgroups;
    const int lane = threadIdx.x;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const long long qg = w % qgroups, br = w / qgroups;
        const int r = (int)(br % splits), b = (int)(br / splits);
        const long long nq = clamped_len(n_queries, b, n);
        const long long mt = clamped_len(n_targets, b, m);
        const int lo = (int)((long long)r * mt / splits), hi = (int)((long long)(r + 1) * mt / splits);      // mt < 2^31, splits <= 1024
        const long long q0 = qg * NN_QUERIES;
        float best[NN_QPT];
        int bj[NN_QPT];
#pragma unroll
        for (int k = 0; k < NN_QPT; ++k) {
            best[k] = INFINITY;
            bj[k] = -1;
        }
        if (q0 < nq && lo < hi) {          // uniform: rows beyond nq and empty ranges skip the search
            // query k of the lane is row q0 + k * WAVE + lane; a row at or beyond nq reads row nq - 1 and its result is discarded below
            const float* qp = queries + (long long)b * n * 3;
            nn_f32x2 qx[NN_PAIRS], qy[NN_PAIRS], qz[NN_PAIRS];
#pragma unroll
            for (int k = 0; k < NN_QPT; ++k) {
                long long i = q0 + k * WAVE + lane;
                i = i < nq ? i : nq - 1;
                const float x = qp[i * 3], y = qp[i * 3 + 1], z = qp[i * 3 + 2];
                if (k & 1) {
                    qx[k / 2].y = x, qy[k / 2].y = y, qz[k / 2].y = z;
                } else {
                    qx[k / 2].x = x, qy[k / 2].x = y, qz[k / 2].x = z;
                }
            }
            const float* tp = targets + (long long)b * m * 3;
            int j = lo;
            for (; j + NN_TILE <= hi; j += NN_TILE) {
                float t[NN_TILE * 3];
#pragma unroll
                for (int c = 0; c < NN_TILE * 3; ++c) t[c] = tp[(long long)j * 3 + c];
#pragma unroll
                for (int u = 0; u < NN_TILE; ++u) nn_step(qx, qy, qz, t[3 * u], t[3 * u + 1], t[3 * u + 2], j + u, best, bj);
            }
            for (; j < hi; ++j) nn_step(qx, qy, qz, tp[(long long)j * 3], tp[(long long)j * 3 + 1], tp[(long long)j * 3 + 2], j, best, bj);
        }
        // every row below n is written: (+inf, -1) at or beyond nq and where nothing was chosen
        const long long row0 = ((long long)b * splits + r) * n;
#pragma unroll
        for (int k = 0; k < NN_QPT; ++k) {
            const long long i = q0 + k * WAVE + lane;
            if (i < n) {
                const bool live = i < nq;
                out_d[row0 + i] = live ? best[k] : INFINITY;
                out_j[row0 + i] = live ? bj[k] : -1;
            }
        }
    }
}

// partial (B, splits, n) -> (B, n): ranges in ascending order, strict <
__global__ __launch_bounds__(NN_REDUCE_BLOCK) void nearest_reduce_kernel(int B, long long n, int splits, const float* __restrict__ part_d,
                                                                         const int32_t* __restrict__ part_j, float* __restrict__ dist2,
                                                                         int32_t* __restrict__ idx) {
    const long long total = (long long)B * n;
    for (long long e = (long long)blockIdx.x * NN_REDUCE_BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * NN_REDUCE_BLOCK) {
        const long long b = e / n, i = e - b * n;
        float best = INFINITY;
        int bj = -1;
        for (int r = 0; r < splits; ++r) {
            const long long at = (b * splits + r) * n + i;
            const float d = part_d[at];
            if (d < best) {
                best = d;
                bj = part_j[at];
            }
        }
        dist2[e] = best;
        idx[e] = bj;
    }
}

hipError_t launch_nearest_points(const NearestArgs& a, hipStream_t stream) {
    const long long qgroups = (a.n + NN_QUERIES - 1) / NN_QUERIES;
    const long long items = (long long)a.B * a.splits * qgroups;
    const bool split = a.splits > 1;
    hipLaunchKernelGGL(nearest_search_kernel, dim3(capped_grid(items, NN_MAX_GRID)), dim3(WAVE), 0, stream, a.B, a.n, a.m, a.splits,
                       a.queries, a.targets, a.n_queries, a.n_targets, split ? a.part_d : a.dist2, split ? a.part_j : a.idx);
    if (hipError_t e = hipGetLastError()) return e;
    if (!split) return hipSuccess;
    const long long blocks = ((long long)a.B * a.n + NN_REDUCE_BLOCK - 1) / NN_REDUCE_BLOCK;
    hipLaunchKernelGGL(nearest_reduce_kernel, dim3(capped_grid(blocks, NN_MAX_GRID)), dim3(NN_REDUCE_BLOCK), 0, stream, a.B, a.n,
                       a.splits, a.part_d, a.part_j, a.dist2, a.idx);
    return hipGetLastError();
}

}  // namespace cnerf
