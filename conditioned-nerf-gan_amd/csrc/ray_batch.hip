// Ray batches (cnerf_render_rays_forward / _backward): sample positions of caller-given rays and the reduction of the sample points'
// position gradients onto the rays.  The rays are any (B,P) list of world origins and directions -- a crop, a random pixel subset, a tile,
// intrinsics with a principal-point offset -- not the R x R pinhole grid the field kernels derive in registers; the field itself then
// runs at explicit points (FIELD_MODE_POINTS), the per-ray stages are those of ray_kernels.hip.
//
// Replaces, for rays the caller formed: the stratified depths (volumetric_rendering.py:100-108) and
// transformed_ray_origins + transformed_ray_directions * z_vals (generators.py:138-142, for the coarse samples as well); autograd of
// that expression with respect to origins / directions (the depths carry no gradient: generators.py:57,111).
//
// The kernels here move 16-28 B per sample point against the field's 0.41 MFLOP: a lane per sample (consecutive lanes write consecutive
// depths and 12-B positions), the ray's six floats are a broadcast load.
#include "cnerf_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

// p = o + d * z per component: the product is rounded, then the sum (no fma: -ffp-contract=off), as fine_sample() and the reference
__device__ __forceinline__ void store_point(const RaySampleArgs& a, long long i, long long ray, float z) {
    const float* o = a.origins + ray * 3;
    const float* d = a.dirs + ray * 3;
    float* p = a.points + i * 3;
    p[0] = o[0] + d[0] * z;
    p[1] = o[1] + d[1] * z;
    p[2] = o[2] + d[2] * z;
}

// coarse samples: z = zl[s] + (u - 0.5) (zl[1] - zl[0]) -- coarse_sample()'s depth, bit for bit -- with u the given tensor, the Philox
// draw of element (b P + p) S + s of stream 0, or 0.5
__global__ __launch_bounds__(256) void ray_sample_coarse_kernel(RaySampleArgs a) {
    const long long n = a.rays * a.S;
    const float dz01 = linspace_at(a.ray_start, a.ray_end, a.S, 1) - linspace_at(a.ray_start, a.ray_end, a.S, 0);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long ray = i / a.S;
        const int s = (int)(i - ray * a.S);
        const float u = a.u_strat ? a.u_strat[i] : a.philox.on ? philox_uniform(a.philox, PHILOX_U_STRAT, (unsigned long long)i) : 0.5f;
        const float zl = linspace_at(a.ray_start, a.ray_end, a.S, s);
        const float off = (u - 0.5f) * dz01;
        const float z = zl + off;
        a.z_out[i] = z;
        store_point(a, i, ray, z);
    }
}

// coarse samples over a per-ray interval: the kernel above with zl[s] = linspace_at(near[ray], far[ray], S, s) -- the same linspace_at, the
// same order of roundings, the same Philox element -- so near / far filled with ray_start / ray_end give its depths bit for bit.  The
// two interval loads are broadcasts: the S lanes of a ray read the same two floats.
__global__ __launch_bounds__(256) void ray_sample_coarse_bounded_kernel(RaySampleArgs a) {
    const long long n = a.rays * a.S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long ray = i / a.S;
        const int s = (int)(i - ray * a.S);
        const float t0 = a.near[ray], t1 = a.far[ray];
        const float dz01 = linspace_at(t0, t1, a.S, 1) - linspace_at(t0, t1, a.S, 0);
        const float u = a.u_strat ? a.u_strat[i] : a.philox.on ? philox_uniform(a.philox, PHILOX_U_STRAT, (unsigned long long)i) : 0.5f;
        const float zl = linspace_at(t0, t1, a.S, s);
        const float off = (u - 0.5f) * dz01;
        const float z = zl + off;
        a.z_out[i] = z;
        store_point(a, i, ray, z);
    }
}

// samples at given depths z (rays, S): the fine pass, and both passes of the backward (which reads the forward's depths)
__global__ __launch_bounds__(256) void ray_sample_at_kernel(RaySampleArgs a) {
    const long long n = a.rays * a.S;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        store_point(a, i, i / a.S, a.z[i]);
}

// grad_origins[ray] += sum_s g_s, grad_dirs[ray] += sum_s z_s g_s over the ray's S samples.  One wave owns a ray: lane l adds samples
// l, l + 64 in that order, then the lanes are summed by a butterfly -- a fixed order, no atomics: two runs agree bit for bit.
__global__ __launch_bounds__(256) void ray_grad_reduce_kernel(RayGradArgs a) {
    const int lane = threadIdx.x & 63;
    const long long ray = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= a.rays) return;
    const float* g = a.grad_points + ray * a.S * 3;
    const float* z = a.z + ray * a.S;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = lane; s < a.S; s += WAVE) {
        const float zs = z[s];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float gk = g[s * 3 + k];
            acc[k] = acc[k] + gk;
            acc[3 + k] = acc[3 + k] + zs * gk;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int d = WAVE / 2; d >= 1; d >>= 1) acc[k] = acc[k] + __shfl_xor(acc[k], d, WAVE);
    if (lane < 3) {
        if (a.grad_origins) a.grad_origins[ray * 3 + lane] += lane == 0 ? acc[0] : lane == 1 ? acc[1] : acc[2];
        if (a.grad_dirs) a.grad_dirs[ray * 3 + lane] += lane == 0 ? acc[3] : lane == 1 ? acc[4] : acc[5];
    }
}

static unsigned sample_blocks(long long n) {
    long long blocks = (n + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

hipError_t launch_ray_sample(const RaySampleArgs& a, hipStream_t stream) {
    if (a.z)
        hipLaunchKernelGGL(ray_sample_at_kernel, dim3(sample_blocks(a.rays * a.S)), dim3(256), 0, stream, a);
    else if (a.near)
        hipLaunchKernelGGL(ray_sample_coarse_bounded_kernel, dim3(sample_blocks(a.rays * a.S)), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(ray_sample_coarse_kernel, dim3(sample_blocks(a.rays * a.S)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_ray_grad_reduce(const RayGradArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(ray_grad_reduce_kernel, dim3((unsigned)((a.rays + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cnerf
