// Connected components of a scalar lattice (cnerf_components_*): every selected point gets the smallest flat index of its component, every
// component its point count, and the lattice can be filtered by them.  include/cnerf.h states the contract (selection, the 14 / 6
// neighbourhoods, labels / sizes / stats); DESIGN.md section 3.25 why the 14 Kuhn neighbours, the invariant and the caps;
// tests/components_common.py restates the result in NumPy.
//
// A union-find in global memory, `labels` itself the parent array, one lane per lattice point:
//
//   init      parent[p] = p where p is selected, else -1; sizes = 0; stats = (0, -1, 0, 0) and the 64-bit key of the largest = 0
//   merge     for each forward kind (3 or 7) whose far end is selected too: unite the two roots (finds halve the paths they walk)
//   flatten   labels[p] = root of p; one integer add per run of lanes of a wave that share a root into sizes[root]; roots counted
//   largest   per root: key = size << 32 | (0xFFFFFFFF - root), a wave maximum, then one 64-bit atomic max per wave that has a root
//   finish    one lane decodes the key into stats[1], stats[2]
//
// The invariant is parent[p] <= p, always.  Every write to a parent in merge is an atomic min at agent scope: values only fall, so there
// is no cycle, a stale read is merely an older ancestor, and the atomic's return value decides who linked.  The root that is left is the
// smallest index of the component whatever the order of arrival, counts are integer sums, the key's maximum is order free: two runs agree
// bit for bit.  Every loop that follows parents carries a cap of n steps (a chain cannot be longer); a lane that hits it stops and ORs a
// bit into stats[3], so a mistake in the protocol is a failed status, never a kernel that spins.  The cap bounds each loop, not the
// kernel's time: at 2^27 points a lane that walked to it would still take long before the bit shows; what it rules out is "for ever".
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int COMP_STATUS_FIND = 1;       // a walk to the root ran into the cap
constexpr int COMP_STATUS_UNITE = 2;      // the link loop of a unite ran into the cap

__device__ __forceinline__ int comp_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int comp_min(int32_t* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void comp_flag(int32_t* stats, int bit) { __hip_atomic_fetch_or(stats + 3, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of selected point x, whose parent was read as `px` (>= 0); -1 if the cap was hit.  On the way every point met is handed its
// grandparent (path halving), by an atomic min as well: lanes that walk one long chain together shorten it for each other.  What a
// parent is lowered to was read as a parent's parent, so it is of the same component once the unites in flight have finished.
__device__ __forceinline__ int comp_find(int32_t* parent, int x, int px, int cap, int32_t* stats) {
    for (int it = 0; px != x; ++it) {
        if (it >= cap) {
            comp_flag(stats, COMP_STATUS_FIND);
            return -1;
        }
        const int gp = comp_load(parent + px);
        if (gp != px) comp_min(parent + x, gp);                    // result unused: the no-return form
        x = px, px = gp;
    }
    return x;
}

__global__ __launch_bounds__(COMP_BLOCK) void comp_init_kernel(CompLabelArgs a) {
    const int p = blockIdx.x * COMP_BLOCK + threadIdx.x;          // n <= 2^27: int holds it, and the padded last block's lanes as well
    if (p == 0) {
        a.stats[0] = 0, a.stats[1] = -1, a.stats[2] = 0, a.stats[3] = 0;
        *a.best = 0ull;
    }
    if (p >= a.d.n) return;
    const bool inside = a.values[p] > a.level;                     // the isosurface's rule: equal to the level and a NaN are outside
    a.labels[p] = inside != (a.invert != 0) ? p : -1;
    a.sizes[p] = 0;
}

// Unites the components of the selected points p and q (parents read as pp, pq).  Both roots, the higher one a linked below the lower one b
// by an atomic min; if a had meanwhile been linked elsewhere (old != a), what it was linked to takes its place: a now hangs below
// min(old, b), and old and b are still to be united.
__device__ __forceinline__ void comp_unite(int32_t* parent, int p, int pp, int q, int pq, int cap, int32_t* stats) {
    int a = comp_find(parent, p, pp, cap, stats), b = comp_find(parent, q, pq, cap, stats);
    for (int it = 0; a >= 0 && b >= 0 && a != b; ++it) {
        if (it >= cap) {
            comp_flag(stats, COMP_STATUS_UNITE);
            return;
        }
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = comp_min(parent + a, b);
        if (old == a) return;
        a = comp_find(parent, old, comp_load(parent + old), cap, stats);      // old < a: a had a parent already, whose root goes on
        b = comp_find(parent, b, comp_load(parent + b), cap, stats);
    }
}

__global__ __launch_bounds__(COMP_BLOCK) void comp_merge_kernel(CompLabelArgs a) {
    const int p = blockIdx.x * COMP_BLOCK + threadIdx.x;
    if (p >= a.d.n) return;
    const int pp = comp_load(a.labels + p);
    if (pp < 0) return;
    const Index3 I = lattice_split(p, a.d.n1, a.d.n2);
    const bool in0 = I.i0 + 1 < a.d.n0, in1 = I.i1 + 1 < a.d.n1, in2 = I.i2 + 1 < a.d.n2;
    const int s0 = a.d.n1 * a.d.n2, s1 = a.d.n2;
    // kind j = d0 + 2 d1 + 4 d2 as in the isosurface; the contiguous axis first, so that its runs are chains before the others join them
    for (int k = 0; k < 7; ++k) {
        const int j = k == 0 ? 4 : k == 1 ? 2 : k == 2 ? 1 : k == 3 ? 6 : k == 4 ? 5 : k == 5 ? 3 : 7;
        if (k >= a.kinds) break;
        if (((j & 1) && !in0) || ((j & 2) && !in1) || ((j & 4) && !in2)) continue;
        const int q = p + (j & 1) * s0 + ((j >> 1) & 1) * s1 + ((j >> 2) & 1);
        const int pq = comp_load(a.labels + q);
        if (pq < 0) continue;
        comp_unite(a.labels, p, comp_load(a.labels + p), q, pq, a.d.n, a.stats);
    }
}

// labels[p] = root, once more by an atomic min (the root is the smallest value a parent can hold): a lane that still walks through p sees
// a shorter chain, never a wrong one.
__global__ __launch_bounds__(COMP_BLOCK) void comp_flatten_kernel(CompLabelArgs a) {
    const int p = blockIdx.x * COMP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    int root = -1;
    if (p < a.d.n) {
        const int pp = comp_load(a.labels + p);
        if (pp >= 0) {
            root = comp_find(a.labels, p, pp, a.d.n, a.stats);
            if (root >= 0 && root != pp) comp_min(a.labels + p, root);
        }
    }
    // runs of neighbouring lanes with one root add once: the head of a run adds the distance to the next head
    const int before = __shfl_up(root, 1);
    const bool head = lane == 0 || before != root;
    const unsigned long long heads = __ballot(head);
    if (head && root >= 0) {
        const unsigned long long above = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
        const int run = above ? __ffsll((long long)above) : WAVE - lane;
        __hip_atomic_fetch_add(a.sizes + root, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long roots = __ballot(root >= 0 && root == p);
    if (lane == 0 && roots) __hip_atomic_fetch_add(a.stats, __popcll(roots), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The sizes are complete (the launch before): the largest component, at equal size the lowest root.
__global__ __launch_bounds__(COMP_BLOCK) void comp_largest_kernel(CompLabelArgs a) {
    const int p = blockIdx.x * COMP_BLOCK + threadIdx.x;
    unsigned long long key = 0ull;
    if (p < a.d.n && a.labels[p] == p) key = ((unsigned long long)(unsigned)a.sizes[p] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)p);
    if (!__ballot(key != 0ull)) return;
    for (int s = WAVE / 2; s > 0; s >>= 1) {
        const unsigned long long o = __shfl_xor(key, s);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) __hip_atomic_fetch_max(a.best, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void comp_finish_kernel(CompLabelArgs a) {
    const unsigned long long key = *a.best;
    if (key == 0ull) return;                                       // no component: (-1, 0) from init
    a.stats[1] = (int32_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    a.stats[2] = (int32_t)(key >> 32);
}

// out = values, but `fill` where a labelled point's component is smaller than min_size or (largest_only) is not the largest.  One load
// and one store per point at the same index: out may be values itself.
__global__ __launch_bounds__(COMP_BLOCK) void comp_filter_kernel(CompFilterArgs a) {
    const int p = blockIdx.x * COMP_BLOCK + threadIdx.x;
    if (p >= a.d.n) return;
    const int root = a.labels[p];
    float v = a.values[p];
    if (root >= 0 && (a.sizes[root] < a.min_size || (a.largest_only && root != a.stats[1]))) v = a.fill;
    a.out[p] = v;
}

hipError_t launch_components_label(const CompLabelArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)a.d.blocks), block(COMP_BLOCK);
    hipLaunchKernelGGL(comp_init_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(comp_merge_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(comp_flatten_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(comp_largest_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(comp_finish_kernel, dim3(1), dim3(1), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_components_filter(const CompFilterArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(comp_filter_kernel, dim3((unsigned)a.d.blocks), dim3(COMP_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cnerf
