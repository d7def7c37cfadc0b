"""Some fp32 field kernels read their packed weights and per-channel vectors through buffer descriptors: a wave-uniform base (the
matrix of the tile's image), the lane part in one register, the group in a scalar offset (csrc/field_common.hpp, WeightStream /
ChanStream).  The kernels that do (BUF in csrc/field_kernel.hip):
  * the plain forwards of a render on per-image folded weights, field_tile_kernel<NT, false, false, false, true, 1 | 2> -- networks of
    FiLM or plain sine layers without residual blocks, through cnerf_render_forward only;
  * field_pw_kernel and field_pw_backward_kernel, the per-point FiLM family (TALLSIREN), on every path.
Every other kernel -- a field query siren(points, z) of the other families (no folded weights there), the storing forward of the
backward, dropout, residual networks, field_backward_kernel -- keeps the flat loads it always had.

What a descriptor can get wrong is a base taken from the wrong image, a record count that is too small for the lane part -- the
hardware then returns zeros without a fault -- and a wrong scalar offset (group index), which the hardware does NOT check: it reads
whatever lies there.  Every output tile and every k-group feeds every output of the network, and a zeroed or foreign 1-KiB group
(32 rows x 8 columns of a matrix) moves the outputs by orders of magnitude more than the gate, so such an error cannot hide.

Which case covers what:
  descriptor code   test_render_reads_each_images_own_weights (all cases: per-image base; TALLSIREN_dgx and SHORTSIREN_FG_Pyrmd have
                    2 and 4 layer-0 input tiles, so layer 0's group index is scalar arithmetic on runtime values),
                    the TALLSIREN cases of test_field_query_matches_float64 and of test_backward_stage_smallest_shape
  flat loads        the other cases of test_field_query_matches_float64, test_several_input_tiles_query and
                    test_backward_stage_smallest_shape: regression cover for the families that share the device functions
                    (WeightStream<false> / ChanStream<false>) and must compute what they did

Shapes: B = 3 images with distinct volumes and FiLM inputs.  Queries: P = 70 points per image = two full 32-point tiles and a ragged
one; the 9 tiles of the call are spread over the 8 bands of the grid (the last band holds two).  Renders: 5 x 5 rays x 14 samples =
350 points per image, 10 full tiles and a ragged one.  H 64 / 128 / 256 are the three instantiations (2 / 4 / 8 output tiles; from 4
on the render kernels keep the next tile's lookups in flight).  Yardstick: the oracle's field in float64 at the same fp32 positions
(oracle.checks.field_fp64) at the 1e-4 gate of the fp32 parity tests (tests/test_gpu_parity.py: rgb and sigma, each on its own
scale).  The backward cases run the stage of tests/test_gpu_field_backward_stage.py -- row by row against float64 at that file's
bounds -- on the smallest of these shapes.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4
B, P = 3, 70

# a FiLM family, a plain-sine / residual family, the per-point FiLM family (field_pw_kernel)
ONE_TILE = ["SHORTSIREN_FG", "SHORTSIREN_FRes", "TALLSIREN"]
# two layer-0 input tiles (features || xyz) and four (a three-level pyramid of 32 + 64 + 32 channels)
MANY_TILES = ["TALLSIREN_dgx", "SHORTSIREN_FG_Pyrmd"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _case(variant, H, seed):
    """(generator on the CPU, its parameters, volume levels, global feature or None, query points)."""
    from test_gpu_field_query_grad import make_case
    gen, vols, glob, pts, _ = make_case(variant, H, B=B, n=P, V=8, seed=seed)
    assert glob is None or not torch.equal(glob[0], glob[1])
    params = {k: v.detach().clone() for k, v in gen.siren.state_dict().items()}
    return gen, params, vols, glob, pts


def _to_device(gen, vols, glob, dev):
    gen.to(dev)
    gen.set_device(dev)
    gen.eval()
    gen.siren.precision = "fp32"
    vd = [v.to(dev) for v in vols]
    fd = vd if len(vd) > 1 else vd[0]
    return (fd, glob.to(dev)) if glob is not None else fd


def _query_vs_fp64(dev, variant, H):
    from oracle import checks as K
    gen, params, vols, glob, pts = _case(variant, H, 31 + H)
    exact = K.field_fp64(variant, params, vols if len(vols) > 1 else vols[0], glob, pts).numpy()
    z = _to_device(gen, vols, glob, dev)
    with torch.no_grad():
        out = gen.siren(pts.to(dev), z)
    torch.cuda.synchronize()
    out = out.cpu().numpy().reshape(exact.shape)
    assert np.isfinite(out).all()
    err = K.rgb_sigma_err(out, exact)
    print(f"{variant} H {H}: rgb_sigma vs float64 {err:.2e}")
    assert err < TOL, (variant, H, err)
    # the images are different work: the outputs of image 0 and image 1 differ by far more than the gate
    assert K.rgb_sigma_err(out[0], exact[1]) > 100 * TOL


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("variant", ONE_TILE)
def test_field_query_matches_float64(dev, variant, H):
    """siren(points, z).  TALLSIREN: field_pw_kernel, descriptors.  SHORTSIREN_FG / SHORTSIREN_FRes: the unfolded field_tile_kernel,
    flat loads (regression cover)."""
    _query_vs_fp64(dev, variant, H)


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("variant", MANY_TILES)
def test_several_input_tiles_query(dev, variant, H):
    """n_in = 2 and 4 through a field query: the unfolded kernel, whose layer-0 weight address stays flat 64-bit arithmetic
    (regression cover; the descriptor form of the same index is covered by the render test below)."""
    _query_vs_fp64(dev, variant, H)


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "SHORTSIREN_F"] + MANY_TILES)
@pytest.mark.parametrize("H", [64, 128, 256])
def test_render_reads_each_images_own_weights(dev, variant, H):
    """The plain forward of a render runs on per-image copies of the weights (rows scaled by the image's FiLM frequencies) and per-image
    starting values: the descriptor's base is a function of the image, and with 2 (TALLSIREN_dgx) or 4 (SHORTSIREN_FG_Pyrmd) input
    tiles layer 0's group index (t * n_in + tk) * 4 + g is scalar arithmetic on runtime values.  3 images, 5 x 5 rays x 14 samples;
    the coarse pass against float64 at the positions the render reports."""
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    from oracle import checks as K
    R, S = 5, 14
    gen, params, vols, glob, _ = _case(variant, H, 41 + H)
    torch.manual_seed(43 + H)
    np.random.seed(43 + H)
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y")
    rng = {"u_strat": torch.rand(B, R * R, S), "u_fine": torch.rand(B, R * R, S)}
    z = _to_device(gen, vols, glob, dev)
    aux = {}
    with torch.no_grad():
        gen(z, cam.to(dev), R, 49.13, 0.25, 1.95, S, True, clamp_mode="relu", nerf_noise=0.0, white_back=True,
            _rng={k: v.to(dev) for k, v in rng.items()}, _aux=aux)
    torch.cuda.synchronize()
    pts = aux["coarse_points"].cpu().reshape(B, R * R * S, 3)
    out = aux["coarse_rgb_sigma"].cpu().numpy().reshape(B, R * R * S, 4)
    assert np.isfinite(out).all()
    exact = K.field_fp64(variant, params, vols if len(vols) > 1 else vols[0], glob, pts).numpy()
    err = K.rgb_sigma_err(out, exact)
    print(f"{variant} H {H} render: coarse rgb_sigma vs float64 {err:.2e}")
    assert err < TOL, (variant, H, err)


@pytest.mark.parametrize("variant", ONE_TILE)
def test_backward_stage_smallest_shape(dev, variant):
    """Storing forward, gradient chain (transposed weight stream) and scatter at H = 64, 3 x 70 points: every stored row against
    float64.  TALLSIREN: field_pw_kernel (storing) and field_pw_backward_kernel, descriptors.  SHORTSIREN_FG / SHORTSIREN_FRes: the
    storing field_tile_kernel and field_backward_kernel, flat loads (regression cover)."""
    from test_gpu_field_backward_stage import run_stage
    run_stage(dev, variant, 64, B, P)
