// Isosurfaces (cnerf_isosurface_*): an indexed triangle mesh of the level set of a scalar lattice, by marching tetrahedra on the Kuhn
// split of every cell.  include/cnerf.h states the algorithm (orderings, arithmetic, orientation); DESIGN.md section 3.19 the workspace
// and why the scan is three launches; tests/isosurface_common.py restates it in NumPy.
//
// One lane per lattice point.  A point OWNS the (up to seven) edges that leave it in a non-negative direction, hence their vertices, and
// the cell whose lowest corner it is, hence its triangles: both streams are compacted in the points' own order by the count / scan / rank
// shape of occupancy.hip -- ballots and popcounts in the wave, LDS across the block's four waves, one block's scan over the block sums.
// No atomics and no block waits for another: two runs agree bit for bit and nothing here can spin.
//
//   classify   code[p] (8 INSIDE bits: own and the seven forward neighbours'), voff[p] / toff[p] = vertices / triangles of the points
//              before p IN ITS BLOCK, block_sums (2, blocks)
//   scan       occupancy.hip's: block_sums -> exclusive block offsets in place, the two totals -> counts
//   emit       vertices and attributes of the point's edges, triangles of its cell; the index of a vertex on an edge owned by point q is
//              block offset + voff[q] + popc(edge mask of q below the edge's kind), read back from q's code -- no 7 n index table
//
// Bandwidth work: 8 L2-served loads of values per point in classify, 9 B per point of workspace written there and read in emit.  The
// lattice rule (flat index split, position of a point) is geom_dev.hpp's, shared with tsdf.hip.
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int ISO_WAVES = ISO_BLOCK / WAVE;

// ---- tables ---------------------------------------------------------------------------------------------------------------------------
// Tetrahedron t of a cell belongs to the axis permutation (a, b, c) in lexicographic order; its vertices are the cell corners with the
// offsets w0 = 0, w1 = e_a, w2 = e_a + e_b, w3 = (1,1,1), a corner offset (d0,d1,d2) written as the number d0 + 2 d1 + 4 d2.
constexpr int ISO_TET_A[6] = {0, 0, 1, 1, 2, 2};
constexpr int ISO_TET_B[6] = {1, 2, 0, 2, 0, 1};
__host__ __device__ constexpr int iso_tet_corner(int t, int x) {
    return x == 0 ? 0 : x == 1 ? (1 << ISO_TET_A[t]) : x == 2 ? ((1 << ISO_TET_A[t]) | (1 << ISO_TET_B[t])) : 7;
}
// [tetrahedron][case]: 1 where the last two indices of the case's triangles are exchanged so that the right-hand normal points from INSIDE
// to outside; case bit x = INSIDE of w_x.  It depends on the parity of the permutation and the case only.  Generated once from the
// geometry (normal against centroid of the outside corners - centroid of the inside corners); tests/test_isosurface_cpu.py checks this very
// text against the oracle's copy, and that copy against the geometry.
constexpr uint8_t ISO_FLIP[6][16] = {
    {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0},
    {0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0},
    {0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0},
    {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0},
    {0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0},
    {0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0},
};
__host__ __device__ constexpr unsigned iso_flip_mask(int t) {
    unsigned m = 0;
    for (int c = 0; c < 16; ++c) m |= (unsigned)ISO_FLIP[t][c] << c;
    return m;
}
// triangles of a tetrahedron case: none for 0 and 15, one where a vertex is alone on its side, two for two against two
__host__ __device__ constexpr int iso_case_triangles(int cs) {
    const int pc = (cs & 1) + ((cs >> 1) & 1) + ((cs >> 2) & 1) + ((cs >> 3) & 1);
    return pc == 0 || pc == 4 ? 0 : pc == 2 ? 2 : 1;
}
__host__ __device__ constexpr int iso_tet_case(int code, int t) {
    int cs = 0;
    for (int x = 0; x < 4; ++x) cs |= ((code >> iso_tet_corner(t, x)) & 1) << x;
    return cs;
}
// triangles (0..12) of a cell by its 8-bit code, bit j = INSIDE of the corner with offset number j
struct IsoCountTable {
    uint8_t n[256];
};
constexpr IsoCountTable iso_count_table() {
    IsoCountTable T{};
    for (int code = 0; code < 256; ++code) {
        int s = 0;
        for (int t = 0; t < 6; ++t) s += iso_case_triangles(iso_tet_case(code, t));
        T.n[code] = (uint8_t)s;
    }
    return T;
}
__constant__ const IsoCountTable ISO_TRIANGLES = iso_count_table();

// the seven edge bits of a code: bit k = the edge of kind k + 1 crosses the level (its far end's INSIDE bit differs from the point's own)
__device__ __forceinline__ unsigned iso_edge_mask(unsigned code) { return ((code >> 1) ^ ((code & 1u) ? 0x7Fu : 0u)) & 0x7Fu; }

__device__ __forceinline__ Index3 iso_index(const IsoDims& d, int p) { return lattice_split(p, d.n1, d.n2); }
// flat distance to the corner with offset number j
__device__ __forceinline__ int iso_step(const IsoDims& d, int j) { return (j & 1) * d.n1 * d.n2 + ((j >> 1) & 1) * d.n2 + ((j >> 2) & 1); }

// Exclusive sums of two small per-lane numbers (nv < 8, nt < 16) over the 256 lanes of the block, and the block's totals: one ballot per
// bit of the numbers, lanes below by popcount, waves before through LDS.
__device__ __forceinline__ void iso_block_scan(int nv, int nt, int& v_before, int& t_before, int& v_total, int& t_total) {
    __shared__ int wave_sum[2][ISO_WAVES];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    int vb = 0, tb = 0, vw = 0, tw = 0;
    for (int b = 0; b < 3; ++b) {
        const unsigned long long m = __ballot((nv >> b) & 1);
        vb += __popcll(m & below) << b;
        vw += __popcll(m) << b;
    }
    for (int b = 0; b < 4; ++b) {
        const unsigned long long m = __ballot((nt >> b) & 1);
        tb += __popcll(m & below) << b;
        tw += __popcll(m) << b;
    }
    if (lane == 0) {
        wave_sum[0][wave] = vw;
        wave_sum[1][wave] = tw;
    }
    __syncthreads();
    v_total = t_total = 0;
    for (int w = 0; w < ISO_WAVES; ++w) {
        const int cv = wave_sum[0][w], ct = wave_sum[1][w];
        vb += w < wave ? cv : 0;
        tb += w < wave ? ct : 0;
        v_total += cv;
        t_total += ct;
    }
    v_before = vb;
    t_before = tb;
}

// Pass 1.  A value is INSIDE iff v > level: a value equal to the level and a NaN are outside.  A neighbour outside the lattice repeats the
// point's own bit, so an edge that leaves the lattice never crosses; a cell that does not exist has no triangles.
__global__ __launch_bounds__(ISO_BLOCK) void iso_classify_kernel(IsoCountArgs a) {
    const int p = blockIdx.x * ISO_BLOCK + threadIdx.x;           // n <= 2^27: int holds it, and the padded last block's lanes as well
    int nv = 0, nt = 0;
    unsigned code = 0;
    if (p < a.d.n) {
        const Index3 I = iso_index(a.d, p);
        const bool own = a.values[p] > a.level;
        const bool in0 = I.i0 + 1 < a.d.n0, in1 = I.i1 + 1 < a.d.n1, in2 = I.i2 + 1 < a.d.n2;
        code = own ? 1u : 0u;
        for (int j = 1; j < 8; ++j) {
            const bool there = ((j & 1) == 0 || in0) && ((j & 2) == 0 || in1) && ((j & 4) == 0 || in2);
            const bool bit = there ? a.values[p + iso_step(a.d, j)] > a.level : own;
            code |= (bit ? 1u : 0u) << j;
        }
        nv = __popc(iso_edge_mask(code));
        nt = in0 && in1 && in2 ? ISO_TRIANGLES.n[code] : 0;
    }
    int vb, tb, vt, tt;
    iso_block_scan(nv, nt, vb, tb, vt, tt);
    if (p < a.d.n) {
        a.code[p] = (uint8_t)code;
        a.voff[p] = vb;
        a.toff[p] = tb;
    }
    if (threadIdx.x == 0) {
        a.block_sums[blockIdx.x] = vt;
        a.block_sums[a.d.blocks + blockIdx.x] = tt;
    }
}

// index of the vertex on the edge of kind k + 1 (k = 0..6) owned by point q
__device__ __forceinline__ int iso_vertex_index(const IsoEmitArgs& a, int q, int k) {
    return a.block_offsets[q / ISO_BLOCK] + a.voff[q] + __popc(iso_edge_mask(a.code[q]) & ((1u << k) - 1u));
}

// Pass 3.  Position of lattice point i on an axis: geom_dev.hpp's lattice_pos, as tsdf.hip forms it.  The vertex of an edge is
// formed from its owner P0 toward the other end P1: t = (level - v0) / (v1 - v0), 0.5 if either value is not finite; P0 + t (P1 - P0)
// per component, every operation rounded on its own.  Rows at or beyond the caller's capacities are not written.
__global__ __launch_bounds__(ISO_BLOCK) void iso_emit_kernel(IsoEmitArgs a) {
    const int p = blockIdx.x * ISO_BLOCK + threadIdx.x;
    if (p >= a.d.n) return;
    const unsigned code = a.code[p];
    const unsigned mask = iso_edge_mask(code);
    const Index3 I = iso_index(a.d, p);
    if (mask) {
        const float v0 = a.values[p];
        const float p0[3] = {lattice_pos(I.i0, a.pitch, a.lo[0]), lattice_pos(I.i1, a.pitch, a.lo[1]), lattice_pos(I.i2, a.pitch, a.lo[2])};
        long long row = (long long)a.block_offsets[blockIdx.x] + a.voff[p];
        for (int k = 0; k < 7; ++k) {
            if (!((mask >> k) & 1u)) continue;
            if ((unsigned long long)row < (unsigned long long)a.max_vertices) {      // (a negative row cannot arise from count's workspace)
                const int j = k + 1;
                const int q = p + iso_step(a.d, j);
                const float v1 = a.values[q];
                const bool finite = fabsf(v0) < INFINITY && fabsf(v1) < INFINITY;       // a NaN compares false
                const float t = finite ? __fdiv_rn(__fsub_rn(a.level, v0), __fsub_rn(v1, v0)) : 0.5f;
                const int i[3] = {I.i0 + (j & 1), I.i1 + ((j >> 1) & 1), I.i2 + ((j >> 2) & 1)};
                for (int c = 0; c < 3; ++c) {
                    const float p1 = lattice_pos(i[c], a.pitch, a.lo[c]);
                    a.vertices[row * 3 + c] = __fadd_rn(p0[c], __fmul_rn(t, __fsub_rn(p1, p0[c])));
                }
                for (int c = 0; c < a.n_attr; ++c) {
                    const float a0 = a.attrs[(size_t)p * a.n_attr + c], a1 = a.attrs[(size_t)q * a.n_attr + c];
                    a.vertex_attrs[row * a.n_attr + c] = __fadd_rn(a0, __fmul_rn(t, __fsub_rn(a1, a0)));
                }
            }
            ++row;
        }
    }
    if (I.i0 + 1 >= a.d.n0 || I.i1 + 1 >= a.d.n1 || I.i2 + 1 >= a.d.n2 || ISO_TRIANGLES.n[code] == 0) return;
    long long row = (long long)a.block_offsets[a.d.blocks + blockIdx.x] + a.toff[p];
    // E(x, y): the vertex on the edge of tetrahedron vertices w_x, w_y -- owned by the lower of the two, its kind their difference
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int w[4] = {iso_tet_corner(t, 0), iso_tet_corner(t, 1), iso_tet_corner(t, 2), iso_tet_corner(t, 3)};
        const unsigned cs = ((code >> w[0]) & 1u) | (((code >> w[1]) & 1u) << 1) | (((code >> w[2]) & 1u) << 2) | (((code >> w[3]) & 1u) << 3);
        const int n_tri = iso_case_triangles((int)cs);
        if (n_tri == 0) continue;
        auto E = [&](int x, int y) {
            const int l = min(x, y), h = max(x, y);
            const int cl = l == 0 ? w[0] : l == 1 ? w[1] : l == 2 ? w[2] : w[3];
            const int ch = h == 0 ? w[0] : h == 1 ? w[1] : h == 2 ? w[2] : w[3];
            return iso_vertex_index(a, p + iso_step(a.d, cl), (ch ^ cl) - 1);
        };
        const bool flip = (iso_flip_mask(t) >> cs) & 1u;
        int tri[2][3];
        if (n_tri == 1) {
            // one vertex m alone on its side, the others p < q < r: (E(m,p), E(m,q), E(m,r))
            const unsigned alone = __popc(cs) == 1 ? cs : (~cs & 15u);
            const int m = __ffs(alone) - 1;
            for (int i = 0; i < 3; ++i) tri[0][i] = E(m, i + (i >= m ? 1 : 0));
        } else {
            // two inside a < b, two outside c < d: the quad E(a,c), E(a,d), E(b,d), E(b,c) as (q0,q1,q2), (q0,q2,q3)
            const unsigned out = ~cs & 15u;
            const int ia = __ffs(cs) - 1, ib = 31 - __clz(cs), ic = __ffs(out) - 1, id = 31 - __clz(out);
            const int q0 = E(ia, ic), q1 = E(ia, id), q2 = E(ib, id), q3 = E(ib, ic);
            tri[0][0] = q0, tri[0][1] = q1, tri[0][2] = q2;
            tri[1][0] = q0, tri[1][1] = q2, tri[1][2] = q3;
        }
        for (int k = 0; k < n_tri; ++k, ++row) {
            if ((unsigned long long)row >= (unsigned long long)a.max_triangles) continue;
            a.triangles[row * 3] = tri[k][0];
            a.triangles[row * 3 + 1] = flip ? tri[k][2] : tri[k][1];
            a.triangles[row * 3 + 2] = flip ? tri[k][1] : tri[k][2];
        }
    }
}

hipError_t launch_iso_count(const IsoCountArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(iso_classify_kernel, dim3((unsigned)a.d.blocks), dim3(ISO_BLOCK), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    return launch_occ_scan(a.block_sums, a.counts, 2, a.d.blocks, stream);      // rows: vertices, triangles
}

hipError_t launch_iso_emit(const IsoEmitArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(iso_emit_kernel, dim3((unsigned)a.d.blocks), dim3(ISO_BLOCK), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cnerf
