// Occupancy grids (cnerf_occupancy_* and cnerf_render_rays_masked_forward): empty-space skipping for forward-only renders of
// caller-given rays.  A grid is G^3 bits per image over an axis-aligned cube; a sample point whose cell's bit is clear is not given to
// the field network -- its rgb_sigma is (0, 0, 0, -inf), which softplus and relu both turn into density 0.  The field kernels are
// untouched: the live points of an image are packed to the front of a buffer (a stable compaction), the field runs on that many explicit
// points, and an expansion puts the values back at their samples.
//
// The reference has no such stage (its render_video / render_pcl / _inference_fixed_camera loops evaluate every sample); DESIGN.md
// section 3.17 states the semantics, tests/occupancy_common.py restates them in NumPy.
//
// All four kernels are bandwidth work of 4 - 28 B per sample point against the field's 0.41 MFLOP; the bit words of an image (at most
// 2 MiB) are re-read through L2, and 32 ray-consecutive points usually hit one or two of them.
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int OCC_BLOCK = 256;            // threads of every block here: four waves
constexpr int OCC_WAVES = OCC_BLOCK / WAVE;

// max that keeps a NaN once it has seen one (fmaxf drops it): v replaces m when it is larger or is a NaN; a NaN m is never replaced
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

// One thread per cell, cells in bit order (ix G + iy) G + iz: the 64 cells of a wave are the two 32-bit words 2 w, 2 w + 1 (G % 4 == 0,
// so G^3 is a multiple of 64 and no wave straddles an image).  The dilated maximum of the cell -- over the cells within `dilate` of it
// on every axis, clipped at the grid, each the maximum of its 8 corners -- is the maximum over the corners [lo, hi + 1]^3 of that cell
// range: one window of at most 10^3 L2-served loads.
__global__ __launch_bounds__(OCC_BLOCK) void occ_build_kernel(OccBuildArgs a) {
    const long long cells = (long long)a.G * a.G * a.G;
    const long long t = (long long)blockIdx.x * OCC_BLOCK + threadIdx.x;
    if (t >= cells * a.B) return;                           // wave-uniform: cells * B is a multiple of 64
    const int b = (int)(t / cells);
    const int cell = (int)(t - (long long)b * cells);
    const int G = a.G, G1 = G + 1, d = a.dilate;
    const int iz = cell % G, iy = (cell / G) % G, ix = cell / (G * G);
    const int x0 = max(ix - d, 0), x1 = min(ix + d, G - 1) + 1;
    const int y0 = max(iy - d, 0), y1 = min(iy + d, G - 1) + 1;
    const int z0 = max(iz - d, 0), z1 = min(iz + d, G - 1) + 1;
    const float* s = a.sigma + (size_t)b * G1 * G1 * G1;
    float m = -INFINITY;
    for (int x = x0; x <= x1; ++x)
        for (int y = y0; y <= y1; ++y) {
            const float* row = s + ((size_t)x * G1 + y) * G1;
            for (int z = z0; z <= z1; ++z) m = nan_max(m, row[z]);
        }
    const unsigned long long mask = __ballot(!(m <= a.threshold));      // a NaN sets the bit
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        uint2 w;
        w.x = (uint32_t)mask;
        w.y = (uint32_t)(mask >> 32);
        *reinterpret_cast<uint2*>(a.bits + (t >> 5)) = w;               // t % 64 == 0: an 8-byte aligned pair of words
    }
}

// Is point p of image b given to the field?  geom_dev.hpp's cell rule per axis: outside the box nothing is skipped, inside the bit decides.
__device__ __forceinline__ bool occ_live(const OccGrid& g, const uint32_t* bits, float x, float y, float z) {
    const float Gf = (float)g.G;
    const float tx = cell_coord(x, g.lo[0], g.inv), ty = cell_coord(y, g.lo[1], g.inv), tz = cell_coord(z, g.lo[2], g.inv);
    if (!(cell_inside(tx, Gf) && cell_inside(ty, Gf) && cell_inside(tz, Gf))) return true;
    const int idx = ((int)floorf(tx) * g.G + (int)floorf(ty)) * g.G + (int)floorf(tz);
    return (bits[idx >> 5] >> (idx & 31)) & 1u;
}

__device__ __forceinline__ const uint32_t* occ_image_bits(const OccGrid& g, int b) {
    return g.bits + (size_t)b * ((size_t)g.G * g.G * g.G / 32);
}

// Pass 1: live points of every chunk of OCC_CHUNK consecutive points of an image -- ballot + popcount per wave, summed over the block's
// rounds in registers and over its four waves by block_wave_sums.  block_counts (B, chunks_per_image).
__global__ __launch_bounds__(OCC_BLOCK) void occ_count_kernel(OccCompactArgs a) {
    __shared__ int wave_sum[OCC_WAVES];
    const int b = blockIdx.y;
    const long long p0 = (long long)blockIdx.x * OCC_CHUNK;
    const uint32_t* bits = occ_image_bits(a.grid, b);
    const float* pts = a.points + (size_t)b * a.n * 3;
    int cnt = 0;
    for (int r = 0; r < OCC_CHUNK / OCC_BLOCK; ++r) {
        const long long p = p0 + r * OCC_BLOCK + threadIdx.x;
        const bool live = p < a.n && occ_live(a.grid, bits, pts[p * 3], pts[p * 3 + 1], pts[p * 3 + 2]);
        cnt += __popcll(__ballot(live));                    // the same number in every lane of the wave
    }
    const int total = block_wave_sums<OCC_WAVES>(cnt, wave_sum).total;
    if (threadIdx.x == 0) a.block_counts[(size_t)b * gridDim.x + blockIdx.x] = total;
}

// Pass 2: one block per image turns its chunk counts into exclusive offsets, in place, and writes counts[b].  256 counts per round: a
// Hillis-Steele scan in LDS, the running total carried from round to round.
__global__ __launch_bounds__(OCC_BLOCK) void occ_scan_kernel(int32_t* block_counts, int32_t* counts, int chunks) {
    __shared__ int buf[2][OCC_BLOCK];
    __shared__ int carry;
    int32_t* c = block_counts + (size_t)blockIdx.x * chunks;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < chunks; base += OCC_BLOCK) {
        const int i = base + threadIdx.x;
        const int own = i < chunks ? c[i] : 0;
        int cur = 0;
        buf[0][threadIdx.x] = own;
        __syncthreads();
        for (int d = 1; d < OCC_BLOCK; d <<= 1) {
            const int v = buf[cur][threadIdx.x] + (threadIdx.x >= d ? buf[cur][threadIdx.x - d] : 0);
            buf[cur ^ 1][threadIdx.x] = v;
            cur ^= 1;
            __syncthreads();
        }
        const int incl = buf[cur][threadIdx.x], before = carry;
        if (i < chunks) c[i] = before + incl - own;
        __syncthreads();                                    // every thread has read carry and buf
        if (threadIdx.x == OCC_BLOCK - 1) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// Pass 3: rank of every point -- its index among the image's live points in ascending order, -1 if skipped -- and the live positions
// packed at the front of live_points.  The chunk's offset from pass 2, then per round of 256 points block_rank: lanes below, waves
// before (LDS), and rounds before (a register).  No atomics: the order is the points' own.
__global__ __launch_bounds__(OCC_BLOCK) void occ_rank_kernel(OccCompactArgs a) {
    __shared__ int wave_cnt[2][OCC_WAVES];
    const int b = blockIdx.y;
    const long long p0 = (long long)blockIdx.x * OCC_CHUNK;
    const uint32_t* bits = occ_image_bits(a.grid, b);
    const float* pts = a.points + (size_t)b * a.n * 3;
    float* out = a.live_points + (size_t)b * a.n * 3;
    int32_t* rank = a.rank + (size_t)b * a.n;
    int base = a.block_counts[(size_t)b * gridDim.x + blockIdx.x];
    for (int r = 0; r < OCC_CHUNK / OCC_BLOCK; ++r) {
        const long long p = p0 + r * OCC_BLOCK + threadIdx.x;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        bool live = false;
        if (p < a.n) {
            x = pts[p * 3];
            y = pts[p * 3 + 1];
            z = pts[p * 3 + 2];
            live = occ_live(a.grid, bits, x, y, z);
        }
        const BlockRank br = block_rank<OCC_WAVES>(live, wave_cnt[r & 1]);      // (two slots: round r + 1 writes the other one while a slow wave still reads this)
        if (p < a.n) {
            const int k = live ? base + br.before : -1;
            rank[p] = k;
            if (live) {
                out[(size_t)k * 3] = x;
                out[(size_t)k * 3 + 1] = y;
                out[(size_t)k * 3 + 2] = z;
            }
        }
        base += br.total;
    }
}

// rgb_sigma[b, i] = live_rgb_sigma[b, rank[b, i]], or (0, 0, 0, -inf) where the point was skipped: one float4 per thread, consecutive
// threads write consecutive rows
__global__ __launch_bounds__(OCC_BLOCK) void occ_expand_kernel(OccExpandArgs a) {
    const long long total = a.n * a.B;
    const float4 fill = make_float4(0.0f, 0.0f, 0.0f, -INFINITY);
    const float4* src = reinterpret_cast<const float4*>(a.live_rgb_sigma);
    float4* dst = reinterpret_cast<float4*>(a.rgb_sigma);
    for (long long i = (long long)blockIdx.x * OCC_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * OCC_BLOCK) {
        const int k = a.rank[i];
        float4 v = fill;
        if (k >= 0) v = src[(i / a.n) * a.n + k];
        dst[i] = v;
    }
}

// ---- per-ray sampling bounds (cnerf_occupancy_ray_bounds) -----------------------------------------------------------------------------
// [near, far] of a ray = the hull of the depths at which it is inside a set cell, widened by pad and clamped to [t_min, t_max]
// (include/cnerf.h states the contract).  Unlike occ_live, a segment of the ray OUTSIDE the cube is empty here: the ray is clipped to
// the cube by a slab test and only cells are looked at.  One lane per ray walks the cells the ray crosses -- a 3-D DDA over the bit
// words, over the whole clipped span, because the last set cell is wanted as well as the first -- and writes its own three results:
// no atomics, nothing shared, two runs agree bit for bit.
//
// Arithmetic, every operation rounded on its own: plane j of axis k is lo[k] + (float)j * cell (j = 0 .. G; cell = side / G rounded
// once on the host), and the ray crosses it at ((plane - o_k) / d_k).  Every crossing depth is formed afresh from its plane index --
// nothing is accumulated from step to step, so the error of a depth does not grow with G: about 4.5 * 2^-23 M in space on the axis
// crossed, M the largest coordinate magnitude among the origin and the cube's corners.  The depths of one axis are monotone in j
// (each operation is), so the walk's depth never decreases.  The cell at the entry comes from the position o + d t0 by occ_live's
// rule, clamped into the grid; where rounding put it one cell behind, the first step has length zero and the walk goes on.
//
// Safe without a division by zero and without an unbounded loop: a component d_k == 0 (+0.0 or -0.0) is never divided by and never
// stepped (the ray misses unless o_k lies in the cube's slab); a NaN or an infinity anywhere in the ray is a miss; every step moves one
// cell index by one inside [0, G), so there are at most 3 G - 2 of them, and the loop counts to 3 G + 3 besides.
__device__ __forceinline__ float occ_plane(float lo, float cell, int j) { return lo + (float)j * cell; }
__device__ __forceinline__ float occ_cross(float lo, float cell, int j, float o, float d) { return (occ_plane(lo, cell, j) - o) / d; }
// cell index of coordinate p on an axis by occ_live's rule, clamped into [0, G) in float (so that no NaN or infinity is converted)
__device__ __forceinline__ int occ_entry_cell(float p, float lo, float inv, int G) {
    return (int)fminf(fmaxf(floorf((p - lo) * inv), 0.0f), (float)(G - 1));
}

__global__ __launch_bounds__(OCC_BLOCK) void occ_ray_bounds_kernel(OccBoundsArgs a) {
    const long long r = (long long)blockIdx.x * OCC_BLOCK + threadIdx.x;
    if (r >= a.P * a.B) return;
    const uint32_t* bits = occ_image_bits(a.grid, (int)(r / a.P));
    const int G = a.grid.G;
    const float cell = a.cell, inv = a.grid.inv;
    const float lx = a.grid.lo[0], ly = a.grid.lo[1], lz = a.grid.lo[2];
    const float ox = a.origins[r * 3], oy = a.origins[r * 3 + 1], oz = a.origins[r * 3 + 2];
    const float dx = a.dirs[r * 3], dy = a.dirs[r * 3 + 1], dz = a.dirs[r * 3 + 2];
    // a NaN compares false: not finite
    bool ok = fabsf(ox) < INFINITY && fabsf(oy) < INFINITY && fabsf(oz) < INFINITY && fabsf(dx) < INFINITY && fabsf(dy) < INFINITY && fabsf(dz) < INFINITY;
    // slab test: [t0, t1] = [t_min, t_max] cut to the depths inside the cube
    float t0 = a.t_min, t1 = a.t_max;
    const int sx = dx > 0.0f ? 1 : dx < 0.0f ? -1 : 0, sy = dy > 0.0f ? 1 : dy < 0.0f ? -1 : 0, sz = dz > 0.0f ? 1 : dz < 0.0f ? -1 : 0;
    auto slab = [&](float lo, float o, float d, int s) {
        if (s == 0) {
            ok = ok && o >= lo && o <= occ_plane(lo, cell, G);
            return;
        }
        const float ta = occ_cross(lo, cell, s > 0 ? 0 : G, o, d), tb = occ_cross(lo, cell, s > 0 ? G : 0, o, d);
        t0 = fmaxf(t0, ta);
        t1 = fminf(t1, tb);
    };
    if (ok) {
        slab(lx, ox, dx, sx);
        slab(ly, oy, dy, sy);
        slab(lz, oz, dz, sz);
    }
    bool hit = false;
    float near = 0.0f, far = 0.0f;
    if (ok && t0 <= t1) {
        int cx = occ_entry_cell(ox + dx * t0, lx, inv, G), cy = occ_entry_cell(oy + dy * t0, ly, inv, G), cz = occ_entry_cell(oz + dz * t0, lz, inv, G);
        // depth at which the ray leaves the current cell through each axis' next plane (never, for an axis it does not move along)
        float nx = sx ? occ_cross(lx, cell, sx > 0 ? cx + 1 : cx, ox, dx) : INFINITY;
        float ny = sy ? occ_cross(ly, cell, sy > 0 ? cy + 1 : cy, oy, dy) : INFINITY;
        float nz = sz ? occ_cross(lz, cell, sz > 0 ? cz + 1 : cz, oz, dz) : INFINITY;
        float t = t0;
        for (int n = 0; n < 3 * G + 3; ++n) {
            const float t_next = fminf(nx, fminf(ny, nz));
            const float t_out = fminf(fmaxf(t_next, t), t1);           // the cell holds the ray over [t, t_out]
            const int idx = (cx * G + cy) * G + cz;
            if ((bits[idx >> 5] >> (idx & 31)) & 1u) {
                if (!hit) near = t;
                hit = true;
                far = t_out;
            }
            if (!(t_next < t1)) break;
            // across the plane that comes first (x before y before z where depths tie), out of the grid: done
            if (nx <= ny && nx <= nz) {
                cx += sx;
                if (cx < 0 || cx >= G) break;
                nx = occ_cross(lx, cell, sx > 0 ? cx + 1 : cx, ox, dx);
            } else if (ny <= nz) {
                cy += sy;
                if (cy < 0 || cy >= G) break;
                ny = occ_cross(ly, cell, sy > 0 ? cy + 1 : cy, oy, dy);
            } else {
                cz += sz;
                if (cz < 0 || cz >= G) break;
                nz = occ_cross(lz, cell, sz > 0 ? cz + 1 : cz, oz, dz);
            }
            t = t_out;
        }
    }
    if (hit) {
        near = fmaxf(a.t_min, near - a.pad);
        far = fminf(a.t_max, far + a.pad);
        hit = far > near;
    }
    a.near[r] = hit ? near : a.t_min;        // a missed ray keeps the whole interval: it is sampled as it always was
    a.far[r] = hit ? far : a.t_max;
    if (a.hit) a.hit[r] = hit ? 1 : 0;
}

hipError_t launch_occ_ray_bounds(const OccBoundsArgs& a, hipStream_t stream) {
    const long long rays = a.P * a.B;
    hipLaunchKernelGGL(occ_ray_bounds_kernel, dim3((unsigned)((rays + OCC_BLOCK - 1) / OCC_BLOCK)), dim3(OCC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_occ_build(const OccBuildArgs& a, hipStream_t stream) {
    const long long threads = (long long)a.B * a.G * a.G * a.G;
    hipLaunchKernelGGL(occ_build_kernel, dim3((unsigned)((threads + OCC_BLOCK - 1) / OCC_BLOCK)), dim3(OCC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_occ_scan(int32_t* block_counts, int32_t* counts, int rows, int chunks, hipStream_t stream) {
    hipLaunchKernelGGL(occ_scan_kernel, dim3(rows), dim3(OCC_BLOCK), 0, stream, block_counts, counts, chunks);
    return hipGetLastError();
}

hipError_t launch_occ_compact(const OccCompactArgs& a, hipStream_t stream) {
    const int chunks = (int)occ_chunks(a.n);
    hipLaunchKernelGGL(occ_count_kernel, dim3(chunks, a.B), dim3(OCC_BLOCK), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = launch_occ_scan(a.block_counts, a.counts, a.B, chunks, stream)) return e;
    hipLaunchKernelGGL(occ_rank_kernel, dim3(chunks, a.B), dim3(OCC_BLOCK), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_occ_expand(const OccExpandArgs& a, hipStream_t stream) {
    const long long blocks = (a.n * a.B + OCC_BLOCK - 1) / OCC_BLOCK;
    hipLaunchKernelGGL(occ_expand_kernel, dim3(capped_grid(blocks, 65536)), dim3(OCC_BLOCK), 0, stream, a);      // the kernel strides over what is beyond
    return hipGetLastError();
}

}  // namespace cnerf
