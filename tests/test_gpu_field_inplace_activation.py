"""The plain forwards of a render on per-image folded weights -- field_tile_kernel<NT, false, false, false, true, 1 | 2, NOVOL> --
run a hidden matrix as hidden_matrix_inplace (csrc/field_kernel.hip): the accumulators of the NT output tiles are the tiles of `y`,
and behind the matrix's last MFMA one pass writes x = sin(2 pi y) over the matrix's own input.  The code runs in renders only
(cnerf_render_forward); a field query siren(points, z) has no folded weights.

What that can get wrong: a tile activated from the wrong accumulator, an input tile overwritten before the last MFMA that reads it, a
depth at which the layer loop runs zero times or once, a starting-value tile (fetched one output tile ahead) that lands behind its
first MFMA.  Every one of them moves the outputs by orders of magnitude more than the gate, so the instrument is accuracy against
float64 on the smallest shapes, both passes of the render (both run the kernel), plus the bit-for-bit batch / single comparison of
tests/test_gpu_field_tile_pipeline.py at the depths that file does not cover.

Accuracy cases: 3 images with distinct volumes / global features / latents, 5 x 5 rays x 14 samples = 350 points per image, 10 full
tiles and a ragged one.  H 64 / 128 / 256 = NT 2 / 4 / 8.  By depth: SingleSIREN_dg (no hidden matrix: the loop body never runs),
DOUBLESIREN_FG (one), SHORTSIREN_FG (three), TALLSIREN_FG (seven); SHORTSIREN_F is the plain-sine form (WFOLD 2); SHORTSIREN is the
family on world positions without a volume (NOVOL), built as tests/global_latent_common.py builds it, its float64 yardstick being
that file's restatement.  Yardstick of the others: oracle.checks.field_fp64 at the positions the render reports, gate 1e-4
(rgb_sigma_err: colour and density each on its own scale), the gate of the fp32 parity tests.

Condition on the inputs: a case is used only if the yardstick's OWN fp32 evaluation is at most 5e-5 (half the gate) from its float64
evaluation on the case's inputs; the test asserts it at the positions the render reported.  The depths of the fine pass are forced
draws (cnerf_rng.fine_z), so the positions of both passes are functions of the seed alone and the condition is checked on a CPU, with
the oracle's render of the same inputs.  Seeds are 51 + H unless SEEDS says otherwise: with 51 + H SHORTSIREN_FG is above half the gate
at H 64 and H 128 (5.1e-5, 5.7e-5 coarse), and the images of SHORTSIREN_F, which has no FiLM input, are within 100 x the gate of each
other (3e-3 .. 8e-3).  The yardstick's own fp32 evaluation, coarse / fine (a CPU; another machine's BLAS moves these by a few per cent):

    variant          H 64               H 128              H 256
    SingleSIREN_dg   2.9e-6 / 2.1e-6    2.5e-6 / 2.3e-6    2.6e-6 / 2.4e-6
    DOUBLESIREN_FG   8.0e-6 / 4.3e-6    5.4e-6 / 6.2e-6    7.2e-6 / 5.6e-6
    SHORTSIREN_FG    3.1e-5 / 3.0e-5    2.9e-5 / 3.7e-5    3.4e-5 / 4.0e-5
    TALLSIREN_FG     1.2e-5 / 1.0e-5    1.1e-5 / 1.3e-5    1.4e-5 / 1.2e-5
    SHORTSIREN_F     3.0e-6 / 3.2e-6    1.8e-6 / 1.6e-6    7.6e-6 / 7.7e-6
    SHORTSIREN       5.1e-6 / 5.0e-6    4.5e-6 / 5.4e-6    5.7e-6 / 5.6e-6

Measured on one MI355X, the kernel's scaled error against float64, coarse / fine (gate 1e-4; the yardstick's own fp32 evaluation on that
machine's CPU was at most 3.7e-5):

    variant          H 64               H 128              H 256
    SingleSIREN_dg   2.8e-6 / 2.9e-6    2.3e-6 / 2.8e-6    2.8e-6 / 2.1e-6
    DOUBLESIREN_FG   6.9e-6 / 6.4e-6    5.8e-6 / 6.7e-6    6.4e-6 / 7.0e-6
    SHORTSIREN_FG    5.3e-5 / 5.6e-5    4.4e-5 / 3.9e-5    5.1e-5 / 4.8e-5
    TALLSIREN_FG     1.2e-5 / 1.5e-5    1.5e-5 / 2.1e-5    2.0e-5 / 2.3e-5
    SHORTSIREN_F     1.3e-5 / 1.4e-5    9.1e-6 / 9.4e-6    1.5e-5 / 1.8e-5
    SHORTSIREN       1.1e-5 / 1.1e-5    6.2e-6 / 8.0e-6    8.2e-6 / 7.9e-6
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the fp32 gate
OWN = 5e-5          # the yardstick's own fp32 evaluation: at most half the gate
B, R, S = 3, 5, 14

VARIANTS = ["SingleSIREN_dg", "DOUBLESIREN_FG", "SHORTSIREN_FG", "TALLSIREN_FG", "SHORTSIREN_F", "SHORTSIREN"]
SEEDS = {("SHORTSIREN_FG", 64): 7, ("SHORTSIREN_FG", 128): 9, ("SHORTSIREN_FG", 256): 7,      # 51 + H: above half the gate
         ("SHORTSIREN_F", 64): 9, ("SHORTSIREN_F", 128): 1, ("SHORTSIREN_F", 256): 7}           # 51 + H: images 0 and 1 within 100 x the gate


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def case_inputs(variant, H, seed=None):
    """Everything on the CPU: (generator, z as the generator takes it, cameras, draws, exact(points), own32(points))."""
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    seed = SEEDS.get((variant, H), 51 + H) if seed is None else seed
    if variant == "SHORTSIREN":
        import global_latent_common as GL
        gen = GL.fresh_generator(H, seed=seed)
        z = torch.randn(B, 32, generator=torch.Generator().manual_seed(seed + 1))
        p32, p64 = GL.cast_params(gen.siren, torch.float32), GL.cast_params(gen.siren, torch.float64)

        def exact(pts):
            with torch.no_grad():
                return GL.field(p64, z.double(), pts.double()).numpy()

        def own32(pts):
            with torch.no_grad():
                return GL.field(p32, z, pts).numpy()
    else:
        from test_gpu_field_query_grad import make_case
        from oracle import checks as K
        from oracle import render_oracle as O
        gen, vols, glob, _, _ = make_case(variant, H, B=B, n=8, V=8, seed=seed)
        params = {k: v.detach().clone() for k, v in gen.siren.state_dict().items()}
        z = (vols[0], glob) if glob is not None else vols[0]

        def exact(pts):
            return K.field_fp64(variant, params, vols[0], glob, pts).numpy()

        def own32(pts):
            with torch.no_grad():
                return O.field_eval(O.FIELD_SPECS[variant], params, vols[0], glob, pts)[0].numpy()
    first = z[0] if isinstance(z, tuple) else z
    assert not torch.equal(first[0], first[1]), "the images need different inputs"
    torch.manual_seed(seed + 2)
    np.random.seed(seed + 2)
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y")
    rng = {"u_strat": torch.rand(B, R * R, S), "u_fine": torch.rand(B, R * R, S)}
    # the depths of the fine pass are forced draws: its positions then do not depend on the coarse pass's outputs, and the condition
    # on the inputs can be checked on a CPU for both passes
    rng["fine_z"] = torch.sort(torch.rand(B, R * R, S) * (1.95 - 0.25) + 0.25, dim=-1).values
    return gen, z, cam, rng, exact, own32


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("variant", VARIANTS)
def test_render_matches_float64(dev, variant, H):
    """Coarse and fine pass of a render against float64 at the positions the render reports."""
    from oracle import checks as K
    gen, z, cam, rng, exact, own32 = case_inputs(variant, H)
    gen.to(dev)
    gen.set_device(dev)
    gen.eval()
    gen.siren.precision = "fp32"
    zd = tuple(t.to(dev) for t in z) if isinstance(z, tuple) else z.to(dev)
    aux = {}
    with torch.no_grad():
        gen(zd, cam.to(dev), R, 49.13, 0.25, 1.95, S, True, clamp_mode="relu", nerf_noise=0.0, white_back=True,
            _rng={k: v.to(dev) for k, v in rng.items()}, _aux=aux)
    torch.cuda.synchronize()
    for pss in ("coarse", "fine"):
        pts = aux[pss + "_points"].cpu().reshape(B, R * R * S, 3)
        out = aux[pss + "_rgb_sigma"].cpu().numpy().reshape(B, R * R * S, 4)
        assert np.isfinite(out).all(), pss
        ex = exact(pts)
        own = K.rgb_sigma_err(own32(pts), ex)
        err = K.rgb_sigma_err(out, ex)
        print(f"{variant} H {H} {pss}: rgb_sigma vs float64 {err:.2e} (the yardstick's own fp32 run {own:.2e})")
        assert own <= OWN, f"unusable inputs: the yardstick's own fp32 run is {own:.2e} from float64 ({variant}, H {H}, {pss})"
        assert err < TOL, (variant, H, pss, err)
        # the images are different work: the outputs of image 0 are far from the float64 values of image 1
        assert K.rgb_sigma_err(out[0], ex[1]) > 100 * TOL, (variant, H, pss)


@pytest.mark.parametrize("variant", ["DOUBLESIREN_FG", "TALLSIREN_FG"])
def test_batch_equals_single(dev, variant):
    """One hidden matrix and seven at H 256: an image rendered inside a batch of 3 equals, bit for bit, the image rendered alone
    (the method and helper of tests/test_gpu_field_tile_pipeline.py, which covers three hidden matrices)."""
    from test_gpu_field_tile_pipeline import _batched_equals_single
    _batched_equals_single(dev, variant, B=3, R=32, S=24, V=16, H=256, seed=25)
