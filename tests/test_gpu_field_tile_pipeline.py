"""The fp32 point-tile kernel keeps state across the tiles a wave walks (the next tile's position and lookups are in flight
under the current tile).  What such a pipeline can get wrong is a value taken from the wrong tile, image or iteration, so
these tests compare the kernel with itself across call shapes: an image rendered inside a batch must equal, bit for bit,
the same image rendered alone with its slice of the draws -- each image has its own folded weights and a point's arithmetic
does not depend on its neighbours -- on shapes where waves loop over several tiles, cross image boundaries and end on
ragged or single tiles.  No tolerance is involved; accuracy stays with the oracle tests (one case here runs at their gate).

Tile arithmetic (the grid is at most 256 blocks x 4 waves; every eighth of the tiles is one band of 128 waves):
  R 64, S 24: 3072 tiles per image, 9216 in a call of 3 = 1152 per band, 9 per wave; bands 2 and 5 cross an image boundary.
  R 32, S 48, one image: 1536 tiles = 192 per band: half of a band's waves own two tiles, the other half one.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DRAWS = ("u_strat", "eps_coarse", "u_fine", "eps_final")
COMPARED = ("coarse_rgb_sigma", "fine_rgb_sigma")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _generator(variant, H, Z, dev, seed):
    import cnerf_amd
    from cnerf_amd.generators import ImplicitGenerator3d
    from oracle import render_oracle as O
    torch.manual_seed(seed)
    np.random.seed(seed)
    has_glob = O.FIELD_SPECS[variant].has_global
    gen = ImplicitGenerator3d(variant, Z if has_glob else 32, 32, 4, H)
    with torch.no_grad():
        gen.siren.final_layer.weight[3] *= 30
    gen.to(dev)
    gen.set_device(dev)
    gen.eval()
    return gen, has_glob


def _batched_equals_single(dev, variant, B, R, S, V, H, Z=64, seed=0):
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    gen, has_glob = _generator(variant, H, Z, dev, seed)
    fvol = (torch.randn(B, 32, V, V, V) * 0.5).to(dev)
    glob = torch.randn(B, Z).to(dev) if has_glob else None
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y").to(dev)
    assert not torch.equal(cam[0], cam[1]), "the images need different cameras"
    P = R * R
    rng = {"u_strat": torch.rand(B, P, S), "eps_coarse": torch.randn(B, P, S), "u_fine": torch.rand(B, P, S),
           "eps_final": torch.randn(B, P, 2 * S)}
    rng = {k: v.to(dev) for k, v in rng.items()}

    def render(sl):
        z = (fvol[sl], glob[sl]) if has_glob else fvol[sl]
        aux = {}
        with torch.no_grad():
            px, dp = gen(z, cam[sl], R, 49.13, 0.25, 1.95, S, True, clamp_mode="softplus", nerf_noise=0.3, white_back=True,
                         _rng={k: rng[k][sl].contiguous() for k in DRAWS}, _aux=aux)
        torch.cuda.synchronize()
        out = {k: aux[k].cpu() for k in COMPARED}
        out["pixels"], out["depth"] = px.cpu(), dp.cpu()
        return out

    batch = render(slice(0, B))
    for k in COMPARED:
        assert torch.isfinite(batch[k]).all(), k
    for b in range(B):
        single = render(slice(b, b + 1))
        for k, v in single.items():
            want = batch[k][b:b + 1]
            assert v.shape == want.shape, (k, v.shape, want.shape)
            differ = int((v != want).sum())
            assert differ == 0, f"{variant} H {H}: image {b} of the batch differs from the image alone in {k} ({differ} elements)"
    # the images really are different work: a kernel that rendered image 0 three times would not pass by accident
    assert not torch.equal(batch["coarse_rgb_sigma"][0], batch["coarse_rgb_sigma"][1])


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "SHORTSIREN_F"])      # FiLM layers / plain sine layers: the two plain forwards
@pytest.mark.parametrize("H", [256, 64])
def test_neighbouring_images_are_independent(dev, variant, H):
    """3 images of different volumes and cameras: 9 tiles per wave, two bands cross an image boundary."""
    _batched_equals_single(dev, variant, B=3, R=64, S=24, V=16, H=H, seed=21)


@pytest.mark.parametrize("shape", [dict(B=3, R=5, S=7, V=9), dict(B=2, R=37, S=33, V=11)])
@pytest.mark.parametrize("H", [256, 64])
def test_ragged_ends(dev, shape, H):
    """Points per image not a multiple of 32 (padded last tile) and a tile count not a multiple of the wave count."""
    _batched_equals_single(dev, "SHORTSIREN_FG", H=H, seed=22, **shape)


@pytest.mark.parametrize("H", [256, 64])
def test_explicit_points_batched_equals_single(dev, H):
    """gen.siren(points, z) runs the same tile loop (explicit positions, shared weights): 3 images x 1000 points, ragged."""
    B, N, V, Z = 3, 1000, 12, 64
    gen, _ = _generator("SHORTSIREN_FG", H, Z, dev, 23)
    fvol = (torch.randn(B, 32, V, V, V) * 0.5).to(dev)
    glob = torch.randn(B, Z).to(dev)
    pts = (torch.rand(B, N, 3) * 0.5 - 0.25).to(dev)
    with torch.no_grad():
        batch = gen.siren(pts, (fvol, glob)).cpu()
        assert torch.isfinite(batch).all()
        for b in range(B):
            single = gen.siren(pts[b:b + 1].contiguous(), (fvol[b:b + 1], glob[b:b + 1])).cpu()
            assert torch.equal(single, batch[b:b + 1]), f"image {b}"
    assert not torch.equal(batch[0], batch[1])


def test_last_tile_of_a_range_matches_oracle(dev):
    """1536 tiles in the call: within every band half of the waves own two tiles and half exactly one (a first tile that is also
    the last, with nothing to fetch ahead).  Against the CPU oracle at the 1e-4 gate of the parity tests (scaled_err)."""
    from test_gpu_parity import _oracle_case
    res = _oracle_case(dev, "SHORTSIREN_FG", B=1, R=32, S=48, V=16, H=256, Z=64, precision="fp32", seed=24)
    print("last tile of a range:", res)
