// V rendered depth maps -> one truncated signed distance lattice: cnerf_tsdf_integrate.  include/cnerf.h states the contract (arithmetic,
// the order of the views, the hidden rule), DESIGN.md section 3.23 the design, tests/tsdf_common.py restates it in NumPy.  The lattice
// goes straight into cnerf_isosurface_* at level 0 with the same lo and pitch.
//
// A gather: one voxel per lane, the views looped inside the lane in ascending order, so a voxel is written by one lane with sums formed
// in a fixed order -- no atomics, no workspace, the same bits for every launch geometry and run.  Lanes of a wave are consecutive i2
// (the fastest axis), so their projections into one view fall on a short line of the image and the depth reads of a wave touch few
// cache lines; the maps of all views (24 x 128 x 128 floats = 1.5 MiB) stay in L2.  The twelve floats of a view's camera and every
// scalar of the arguments are the same address for every lane: they arrive through the scalar data path (the pointers are __restrict__
// and the view index is uniform), and the vector operations take them as scalar operands.
//
// Positions and camera coordinates are formed per voxel from its indices, never stepped, by geom_dev.hpp's rules (isosurface.hip's lattice).
#include "cnerf_dev.hpp"
#include "geom_dev.hpp"
#include "cnerf_kernels.hpp"

namespace cnerf {

constexpr int TSDF_BLOCK = 256;                    // four waves; a block owns 256 consecutive voxels of the flat lattice

template <bool COLOR>
__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_kernel(TsdfArgs a, const float* __restrict__ depth, const float* __restrict__ colors,
                                                          const float* __restrict__ cams, float* __restrict__ tsdf,
                                                          int32_t* __restrict__ weight, float* __restrict__ rgb) {
    const int total = a.n0 * a.n1 * a.n2;                                   // <= 2^27
    const int e = (int)blockIdx.x * TSDF_BLOCK + (int)threadIdx.x;
    if (e >= total) return;
    const Index3 I = lattice_split(e, a.n1, a.n2);
    const float p[3] = {lattice_pos(I.i0, a.pitch, a.lo[0]), lattice_pos(I.i1, a.pitch, a.lo[1]), lattice_pos(I.i2, a.pitch, a.lo[2])};
    const int R = a.R;
    const size_t RR = (size_t)R * R;
    const float half = __fmul_rn(0.5f, (float)(R - 1));
    const float fR = (float)R;
    float sum = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    int n = 0, hidden = 0, cn = 0;
    for (int w = 0; w < a.V; ++w) {                                          // w is uniform: M comes through scalar loads
        const float* M = cams + (size_t)w * 16;
        float q[3], u, v;
        const float z = cam_depth(M, p, q);
        if (!(z > 0.0f)) continue;                                           // behind the camera, or a NaN
        cam_pixel(q, z, M, a.focal, half, u, v);
        if (!(-1.0f < u && u < fR && -1.0f < v && v < fR)) continue;
        const int col = (int)rintf(u), row = (int)rintf(v);
        if (col < 0 || col >= R || row < 0 || row >= R) continue;            // (-1, -0.5] and [R - 0.5, R) round outside
        const size_t pix = (size_t)row * R + col;
        const float d = depth[(size_t)w * RR + pix];
        if (a.z_min < d && d < a.z_max) {                                    // a surface pixel
            const float s = __fsub_rn(z, d) / a.trunc;                       // positive behind the surface
            if (s > 1.0f) {
                ++hidden;                                                    // occluded: no observation
            } else {
                if (COLOR && s >= -1.0f) {
                    const ViewColor cv = view_color_at(colors, a.color_layout, w, RR, pix);
                    c0 = __fadd_rn(c0, view_color(cv, 0, a.color_scale, a.color_offset));
                    c1 = __fadd_rn(c1, view_color(cv, 1, a.color_scale, a.color_offset));
                    c2 = __fadd_rn(c2, view_color(cv, 2, a.color_scale, a.color_offset));
                    ++cn;
                }
                sum = __fadd_rn(sum, fmaxf(s, -1.0f));
                ++n;
            }
        } else if (d == d && a.carve) {                                      // a background pixel (+-inf included); a NaN says nothing
            sum = __fadd_rn(sum, -1.0f);
            ++n;
        }
    }
    tsdf[e] = n > 0 ? sum / (float)n : (a.hidden_min > 0 && hidden >= a.hidden_min ? 1.0f : a.unseen);
    if (weight) weight[e] = n > 0 ? n : -hidden;
    if (COLOR && rgb) {
        const float k = (float)cn;
        float* o = rgb + (size_t)e * 3;
        o[0] = cn > 0 ? c0 / k : 0.0f;
        o[1] = cn > 0 ? c1 / k : 0.0f;
        o[2] = cn > 0 ? c2 / k : 0.0f;
    }
}

hipError_t launch_tsdf_integrate(const TsdfArgs& a, hipStream_t stream) {
    const int total = a.n0 * a.n1 * a.n2;
    const dim3 grid((unsigned)((total + TSDF_BLOCK - 1) / TSDF_BLOCK)), block(TSDF_BLOCK);
    if (a.colors && a.rgb)          // colours that nobody asked the mean of are not read
        hipLaunchKernelGGL(tsdf_kernel<true>, grid, block, 0, stream, a, a.depth, a.colors, a.cam2world, a.tsdf, a.weight, a.rgb);
    else
        hipLaunchKernelGGL(tsdf_kernel<false>, grid, block, 0, stream, a, a.depth, a.colors, a.cam2world, a.tsdf, a.weight, a.rgb);
    return hipGetLastError();
}

}  // namespace cnerf
