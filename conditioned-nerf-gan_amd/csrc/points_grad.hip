// Gradient of a field query w.r.t. its positions (cnerf_field_query_backward, cnerf_feature_points_grad) and the materialised
// dropout keep decisions of a point range (cnerf_dropout_keep).  Nothing here runs on the render path.
//
// d loss / d x of a query point has two terms:
//   lookup  sum over levels and channels of g_feat[c] * d feat_c / d x through the trilinear weights of F.grid_sample
//           (siren.py:555-571; ATen grid_sampler_3d_backward, border padding, align_corners=False): per axis
//           d ic / d x = (V / 2) / half_voxel, and zero where the unnormalised coordinate sits at or beyond the clamp
//           ("borders are considered out of bounds");
//   direct  the xyz columns of layer 0's input (TALLSIREN_dgx's xyz tile, TALLSIREN's layer 0).
// g_feat / g_xyz are the input gradient of one weight matrix, formed here from the gradient slab the chunk body left behind
// (input_grad_kernel): g_in = (g (.) f) W for W (K, k_in) row-major as nn.Linear holds it -- FiLM layer 0: g = d/d arg_0 and
// f = freq_0, a plain sine layer: f = 1, the per-point FiLM family: g = d/d (Wm1 feat + bm1) against Wm1 and
// g = d/d (W_0 xyz + b_0) against W_0.  The slab is fp32 rows (exact backward) or a TB16 fp16 slab with its inverse scale.
#include "cnerf_dev.hpp"
#include "cnerf_kernels.hpp"
#include "bwd16.hpp"

namespace cnerf {

namespace {

// Block: 32 points x 64 columns of g_in, 256 threads (point tid / 8, columns tid % 8 + 8 e); K in chunks of 32 through LDS.
// fp32 FMA on the vector units: K x k_in <= 256 x 227 products per point, a few percent of the chain's work.
__global__ __launch_bounds__(256) void input_grad_kernel(InputGradArgs a) {
    __shared__ float gs[32][33];   // [k][point]
    __shared__ float ws[32][64];   // [k][column]
    const int tid = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * 32;
    const int j0 = blockIdx.y * 64;
    const int tp = tid >> 3, tc = tid & 7;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    for (int k0 = 0; k0 < a.K; k0 += 32) {
        for (int i = tid; i < 32 * 32; i += 256) {
            const int pp = i >> 5, kk = i & 31;
            const long long p = p0 + pp;
            float v = 0.0f;
            if (p < a.n) {
                v = a.g32 ? a.g32[p * a.ldg + k0 + kk]
                          : (float)reinterpret_cast<const _Float16*>(a.g16)[tb16_index(p >> 5, a.g_ct, (k0 + kk) >> 5, (int)(p & 31), kk)];
                if (a.f) v *= a.f[k0 + kk];
            }
            gs[kk][pp] = v;
        }
        for (int i = tid; i < 32 * 64; i += 256) {
            const int kk = i >> 6, jj = i & 63;
            ws[kk][jj] = j0 + jj < a.k_in ? a.W[(size_t)(k0 + kk) * a.k_in + j0 + jj] : 0.0f;
        }
        __syncthreads();
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
            const float gv = gs[kk][tp];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(gv, ws[kk][tc + 8 * e], acc[e]);
        }
        __syncthreads();
    }
    const long long p = p0 + tp;
    if (p >= a.n) return;
    const float s = a.inv_scale ? *a.inv_scale : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int j = j0 + tc + 8 * e;
        if (j < a.k_in) a.out[p * a.ldo + j] = acc[e] * s;
    }
}

// one axis of a lookup: floor index, fractional weights (as trilinear_corners forms them) and d ic / d x (0 at the clamp)
__device__ __forceinline__ void axis_grad(float p, float half_voxel, int V, int& i0, float& lo, float& hi, float& dic) {
    unnormalize(p, half_voxel, V, i0, lo, hi);
    const float ic = ((p / half_voxel + 1.0f) * (float)V - 1.0f) / 2.0f;
    dic = (ic <= 0.0f || ic >= (float)(V - 1)) ? 0.0f : (float)V * 0.5f / half_voxel;
}

// 32 lanes per point (channels lane, lane + 32, ...), 8 points per block; every corner line is read as 128-byte rows.
__global__ __launch_bounds__(256) void points_lookup_grad_kernel(PointsGradArgs a) {
    const int lane = threadIdx.x & 31;
    const long long p = (long long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const bool valid = p < a.n;
    const long long pc = valid ? p : a.n - 1;
    const float px = a.points[pc * 3 + 0], py = a.points[pc * 3 + 1], pz = a.points[pc * 3 + 2];
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    int coff = 0;
    for (int l = 0; l < a.n_levels; ++l) {
        const int V = a.lvl_V[l], Cl = a.lvl_C[l];
        int ix, iy, iz;
        float lx, hx, ly, hy, lz, hz, dx, dy, dz;
        axis_grad(px, a.half_voxel, V, ix, lx, hx, dx);
        axis_grad(py, a.half_voxel, V, iy, ly, hy, dy);
        axis_grad(pz, a.half_voxel, V, iz, lz, hz, dz);
        const int ix1 = min(ix + 1, V - 1), iy1 = min(iy + 1, V - 1), iz1 = min(iz + 1, V - 1);
        const float* g = a.gfeat + pc * a.ldf + coff;
        float lxs = 0.0f, lys = 0.0f, lzs = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int xx = (k & 1) ? ix1 : ix, yy = (k & 2) ? iy1 : iy, zz = (k & 4) ? iz1 : iz;
            const float wx = (k & 1) ? lx : hx, wy = (k & 2) ? ly : hy, wz = (k & 4) ? lz : hz;
            const float* v = a.lvl_vol[l] + ((size_t)(zz * V + yy) * V + xx) * Cl;
            float d = 0.0f;
            for (int c = lane; c < Cl; c += 32) d = __builtin_fmaf(g[c], v[c], d);
            const float sx = (k & 1) ? 1.0f : -1.0f, sy = (k & 2) ? 1.0f : -1.0f, sz = (k & 4) ? 1.0f : -1.0f;
            lxs = __builtin_fmaf(d, sx * wy * wz, lxs);
            lys = __builtin_fmaf(d, wx * sy * wz, lys);
            lzs = __builtin_fmaf(d, wx * wy * sz, lzs);
        }
        gx = __builtin_fmaf(lxs, dx, gx);
        gy = __builtin_fmaf(lys, dy, gy);
        gz = __builtin_fmaf(lzs, dz, gz);
        coff += Cl;
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        gx += __shfl_xor(gx, off, 32);
        gy += __shfl_xor(gy, off, 32);
        gz += __shfl_xor(gz, off, 32);
    }
    if (lane != 0 || !valid) return;
    if (a.gxyz) {
        gx += a.gxyz[pc * a.ldx + 0];
        gy += a.gxyz[pc * a.ldx + 1];
        gz += a.gxyz[pc * a.ldx + 2];
    }
    float* o = a.grad_points + pc * 3;
    o[0] += gx;
    o[1] += gy;
    o[2] += gz;
}

// keep bytes (n_drop, n_points, H) of points [gp0, gp0 + n_points) of a call: the words drop_factors() draws in the kernels
__global__ __launch_bounds__(256) void drop_keep_kernel(PhiloxKey k, uint32_t stream_id, uint32_t thresh, int n_drop, int H,
                                                        unsigned long long gp0, long long n_points, uint8_t* mask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int q = H / 4;
    if (i >= (long long)n_drop * n_points * q) return;
    const int c0 = (int)(i % q) * 4;
    const long long r = i / q;
    const long long pl = r % n_points;
    const int d = (int)(r / n_points);
    const unsigned long long idx = (((gp0 + (unsigned long long)pl) * (unsigned long long)n_drop + d) * H + c0) >> 2;
    uint32_t o[4];
    philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), stream_id, k.offset, k.seed_lo, k.seed_hi, o);
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= (o[e] >= thresh ? 1u : 0u) << (8 * e);
    *reinterpret_cast<uint32_t*>(mask + ((size_t)d * n_points + pl) * H + c0) = m;
}

}  // namespace

hipError_t launch_input_grad(const InputGradArgs& a, hipStream_t stream) {
    if (a.n < 1) return hipSuccess;
    hipLaunchKernelGGL(input_grad_kernel, dim3((unsigned)((a.n + 31) / 32), (unsigned)((a.k_in + 63) / 64)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_points_lookup_grad(const PointsGradArgs& a, hipStream_t stream) {
    if (a.n < 1) return hipSuccess;
    hipLaunchKernelGGL(points_lookup_grad_kernel, dim3((unsigned)((a.n + 7) / 8)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_drop_keep(const PhiloxKey& k, uint32_t stream_id, uint32_t thresh, int n_drop, int H, unsigned long long gp0,
                            long long n_points, uint8_t* mask, hipStream_t stream) {
    const long long total = (long long)n_drop * n_points * (H / 4);
    if (total < 1) return hipSuccess;
    hipLaunchKernelGGL(drop_keep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, k, stream_id, thresh, n_drop, H, gp0,
                       n_points, mask);
    return hipGetLastError();
}

}  // namespace cnerf
