// Mapping-network stage of the per-point FiLM family's exact fp32 backward (cnerf_pfilm_backward_finish): what follows
// field_pw_backward_kernel on one chunk of n rows.  The chunk matrices are row-major fp32 as that kernel left them:
//     G (n, K2 = 2 L H) = d / d (Wm2 m + bm2),   m (n, 256) = LeakyReLU_0.2(Wm1 feat + bm1),   g_pre_0 (n, H),   points (n, 3).
//
// pfilm_gm32_kernel:  g_mpre (n, 256) = (G Wm2) (.) (m > 0 ? 1 : 0.2)   and, chained on the accumulators,   d feat (n, 32) = g_mpre Wm1.
// v_mfma_f32_32x32x2_f32 computes D[i][j] += A[i][k] B[k][j], lane (c = lane & 31, p = lane >> 5) supplying A[c][p] and B[p][c] and
// holding D[8 g + 4 p + e][c] in register 4 g + e.  Here i = the 256 hidden channels of the mapping network (eight accumulator tiles
// resident per 32-point tile), j = the point, k = a column of G: B = G^T, so lane (c, p) reads its own row of G, 16 bytes at columns
// 8 q + 4 p .. + 3 per group q of eight columns, and register e of that piece is the B operand of k-step (q, e), which contracts the
// columns 8 q + e (p = 0) and 8 q + 4 + e (p = 1).  That k-permutation is folded into the packed order of Wm2 (pack_pfilm_map_kernel):
//     packed[(q * 8 + t) * 64 + lane][e] = Wm2[8 q + 4 p + e][32 t + c]
// so one 16-byte LDS read per (q, t) feeds four k-steps.  The loop is k-outer: every element of G is read once.  The packed stream is
// shared by the block's four waves through LDS: stages of GM_Q groups (32 columns of G, 32 KiB) parked by LDS-DMA, double-buffered,
// one barrier per stage behind a written-out wait_vmcnt<0>() as in weight_grad_kernel.
// The accumulator layout of the first product is the B layout of the second (lane (c, p) holds channels 32 t + 8 g + 4 p + e of
// point c: again the pair (e, 4 + e) per k-step), so d feat = g_mpre Wm1 runs on the masked accumulators with A read from
//     packed_wm1[((t * 4 + g) * 4 + e) * 64 + lane] = Wm1[32 t + 8 g + 4 p + e][c]
// and both results leave as 16-byte row pieces.  Rows past the end of the chunk: the G address is clamped to row n - 1, the loaded
// values are replaced by zeros, nothing is stored -- no byte beyond row n is read or written.
#include "cnerf_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int GM_Q = 4;                          // groups of eight G columns per LDS stage
constexpr int GM_STAGE_F4 = GM_Q * 8 * 64;       // float4 per stage of packed Wm2 (32 KiB)

struct PfilmGmArgs {
    const float* packed;   // packed Wm2 (K2 * 256 floats) then packed Wm1 (256 * 32 floats)
    const float* G;        // (n, K2)
    const float* m;        // (n, 256)
    float* g_mpre;         // (n, 256)
    float* d_feat;         // (n, 32)
    long long n;
    int K2;
};

// one 32-point tile per wave, two blocks per CU (204 registers, 64 KiB of LDS each)
__global__ __launch_bounds__(256, 2) void pfilm_gm32_kernel(PfilmGmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* lds4 = reinterpret_cast<f32x4*>(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int c = lane & 31, p = lane >> 5;
    const int stages = a.K2 / (8 * GM_Q);
    const f32x4* src4 = reinterpret_cast<const f32x4*>(a.packed);

    const long long row = ((long long)blockIdx.x * 4 + wave) * 32 + c;
    const bool valid = row < a.n;
    const size_t row_c = (size_t)(valid ? row : a.n - 1);      // rows past the end: the last row's address, zeroed values, no store
    const float* grow = a.G + row_c * a.K2 + 4 * p;

    auto dma_stage = [&](int s, int buf) {       // 32 pieces of 1 KiB, eight per wave: a linear copy
#pragma unroll
        for (int i = 0; i < GM_STAGE_F4 / 256; ++i) {
            const int q = wave_u * (GM_STAGE_F4 / 256) + i;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src4 + (size_t)s * GM_STAGE_F4 + q * 64 + lane),
                                             (__attribute__((address_space(3))) void*)(lds4 + buf * GM_STAGE_F4 + q * 64), 16, 0, 0);
        }
    };
    auto load_g = [&](int s, f32x4 (&g)[GM_Q]) {
#pragma unroll
        for (int q = 0; q < GM_Q; ++q) g[q] = *reinterpret_cast<const f32x4*>(grow + 8 * (GM_Q * s + q));
    };

    f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    f32x4 g_next[GM_Q];
    dma_stage(0, 0);
    load_g(0, g_next);
    int cur = 0;
    for (int s = 0; s < stages; ++s) {
        f32x4 g_cur[GM_Q];
        wait_vmcnt<0>();                          // this wave's pieces of stage s (and its G pieces) have landed ...
#pragma unroll
        for (int q = 0; q < GM_Q; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) g_cur[q][e] = valid ? g_next[q][e] : 0.0f;
        __syncthreads();                          // ... and everybody's; the other buffer is free
        if (s + 1 < stages) {
            dma_stage(s + 1, cur ^ 1);
            load_g(s + 1, g_next);
        }
        const f32x4* w4 = lds4 + cur * GM_STAGE_F4 + lane;
#pragma unroll
        for (int q = 0; q < GM_Q; ++q) {
            f32x4 w[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) w[t] = w4[(q * 8 + t) * 64];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[t][e], g_cur[q][e], acc[t], 0, 0, 0);
        }
        cur ^= 1;
    }

    // epilogue: LeakyReLU' from the m rows, g_mpre out, d feat = g_mpre Wm1 on the masked accumulators
    const float* wm1 = a.packed + (size_t)a.K2 * 256 + lane;
    f32x16 df;
#pragma unroll
    for (int r = 0; r < 16; ++r) df[r] = 0.0f;
    const size_t mrow = row_c * 256 + 4 * p;
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 mv = *reinterpret_cast<const f32x4*>(a.m + mrow + 32 * t + 8 * g);
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[t][4 * g + e] * (mv[e] > 0.0f ? 1.0f : 0.2f);
            if (valid) *reinterpret_cast<f32x4*>(a.g_mpre + mrow + 32 * t + 8 * g) = v;
#pragma unroll
            for (int e = 0; e < 4; ++e) df = __builtin_amdgcn_mfma_f32_32x32x2f32(wm1[((t * 4 + g) * 4 + e) * 64], v[e], df, 0, 0, 0);
        }
    if (valid)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = df[4 * g + e];
            *reinterpret_cast<f32x4*>(a.d_feat + (size_t)row * 32 + 8 * g + 4 * p) = v;
        }
}

hipError_t launch_pfilm_gm32(const float* packed_map, const float* G, const float* m, long long n, int K2, float* g_mpre, float* d_feat,
                             hipStream_t stream) {
    if (n < 1 || n > (1ll << 38) || K2 < 8 * GM_Q || K2 % (8 * GM_Q)) return hipErrorInvalidValue;
    PfilmGmArgs a{packed_map, G, m, g_mpre, d_feat, n, K2};
    const int lds_bytes = 2 * GM_STAGE_F4 * 16;
    if (hipError_t e = hipFuncSetAttribute((const void*)pfilm_gm32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)) return e;
    hipLaunchKernelGGL(pfilm_gm32_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), lds_bytes, stream, a);
    return hipGetLastError();
}

// packed_map = [Wm2 in the k-permuted A-operand order above: K2 * 256 floats][Wm1 in the chained product's: 256 * 32 floats]
__global__ void pack_pfilm_map_kernel(const float* __restrict__ wm1, const float* __restrict__ wm2, int K2, float* __restrict__ dst) {
    const long long n2 = (long long)K2 * 256, total = n2 + 256 * 32;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        if (i < n2) {
            const int e = (int)(i & 3), lane = (int)((i >> 2) & 63), t = (int)((i >> 8) & 7);
            const long long q = i >> 11;
            const int c = lane & 31, p = lane >> 5;
            dst[i] = wm2[(size_t)(8 * q + 4 * p + e) * 256 + 32 * t + c];
        } else {
            const int j = (int)(i - n2), lane = j & 63, step = j >> 6;
            const int c = lane & 31, p = lane >> 5;
            const int ch = 32 * (step >> 4) + 8 * ((step >> 2) & 3) + 4 * p + (step & 3);
            dst[i] = wm1[ch * 32 + c];
        }
    }
}
hipError_t launch_pack_pfilm_map(const float* wm1, const float* wm2, int K2, float* dst, hipStream_t stream) {
    const long long total = (long long)K2 * 256 + 256 * 32;
    hipLaunchKernelGGL(pack_pfilm_map_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, wm1, wm2, K2, dst);
    return hipGetLastError();
}

// Layer 0 reads the sample position: dW_0 (H, 3) += g_pre_0^T points, db_0 (H) += column sums of g_pre_0, over n points.  K = 3 is no
// MFMA shape: like head_grad32_kernel, thread c of a block owns channel c (g[point][c] is a coalesced row read, the position a
// broadcast) and the blocks split the points.
__global__ __launch_bounds__(256) void layer0_grad32_kernel(const float* __restrict__ g, const float* __restrict__ pts, long long n, int H,
                                                            float* __restrict__ dW, float* __restrict__ db) {
    const int c = threadIdx.x;
    if (c >= H) return;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long n0 = (long long)blockIdx.x * per, n1 = n0 + per < n ? n0 + per : n;
    float acc[3] = {0.f, 0.f, 0.f}, cs = 0.f;
    for (long long q = n0; q < n1; ++q) {
        const float gv = g[q * H + c];
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[r] = __builtin_fmaf(gv, pts[q * 3 + r], acc[r]);
        cs += gv;
    }
    if (dW)
#pragma unroll
        for (int r = 0; r < 3; ++r) atomicAdd(dW + (size_t)c * 3 + r, acc[r]);
    if (db) atomicAdd(db + c, cs);
}
hipError_t launch_layer0_grad32(const float* g, const float* pts, long long n, int H, float* dW, float* db, hipStream_t stream) {
    if (H > 256 || n < 1) return hipErrorInvalidValue;
    long long blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(layer0_grad32_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, g, pts, n, H, dW, db);
    return hipGetLastError();
}

}  // namespace cnerf
