"""Voxel grids of point clouds and their first-hit pictures, no GPU: the host code's exports, workspace sizes and refusals; the NumPy
statements of the two contracts (tests/voxelize_common.py) against float64 statements of what the reference computes."""
import ctypes

import numpy as np
import pytest

import voxelize_common as VC

ENTRIES = ("cnerf_voxelize_bytes", "cnerf_voxelize", "cnerf_voxel_first_hit")
F = np.float32


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def test_exports_and_prototypes(L):
    """The five new public symbols: three entries of the C ABI and the two functions of ops over them."""
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10 and "#define CNERF_ABI_VERSION 10" in header
    import cnerf_amd
    assert callable(cnerf_amd.ops.voxelize) and callable(cnerf_amd.ops.voxel_first_hit)
    assert cnerf_amd.voxels.voxelize_cloud and cnerf_amd.voxels.voxel_surface_render and cnerf_amd.voxels.save_voxel_npz


def test_workspace_bytes(L):
    lib = L.lib()
    nb = ctypes.c_size_t(7)
    for B, G in ((1, 2), (3, 5), (2, 64), (8, 128), (1, 256)):
        assert lib.cnerf_voxelize_bytes(B, G, ctypes.byref(nb)) == 0, lib.cnerf_last_error()
        need = 32 * B * G ** 3                                       # a count and three sums, 64 bits each, per cell
        assert need <= nb.value < need + 256 and nb.value % 256 == 0
    assert lib.cnerf_voxelize_bytes(1, 2, None) == 0                 # the size pointer is optional


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t()
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def f3(v):
        return None if v is None else (ctypes.c_float * 3)(*v)

    def vox(B=2, n=100, stride=6, points=fake, n_points=None, G=8, lo=(-0.6, -0.6, -0.6), side=1.2, clip=1e-4, layout=0, voxels=fake, counts=None,
            ws=fake):
        return lib.cnerf_voxelize(B, n, stride, points, n_points, G, f3(lo), side, clip, layout, voxels, counts, ws, None)

    for kw, word in ((dict(B=0), "B=0"), (dict(B=-3), "B=-3"), (dict(n=0), "n=0"), (dict(n=-1), "n=-1"), (dict(n=2 ** 28), "2^28"),
                     (dict(stride=5), "stride=5"), (dict(stride=0), "stride=0"), (dict(G=1), "G=1"), (dict(G=257), "G=257"), (dict(G=-4), "G=-4"),
                     (dict(side=0.0), "side"), (dict(side=-1.0), "side"), (dict(side=inf), "side"), (dict(side=nan), "side"),
                     (dict(side=1e-45), "not finite"), (dict(side=1e-38, G=256), "not finite"),      # (float)G / side overflows
                     (dict(lo=(0.0, inf, 0.0)), "lo[1]"), (dict(lo=(nan, 0.0, 0.0)), "lo[0]"), (dict(lo=(0.0, 0.0, -inf)), "lo[2]"), (dict(lo=None), "lo"),
                     (dict(clip=nan), "clip_margin"), (dict(clip=0.6), "clip_margin"), (dict(clip=0.7), "clip_margin"), (dict(clip=inf), "clip_margin"),
                     (dict(layout=2), "layout=2"), (dict(layout=-1), "layout=-1"),
                     (dict(points=None), "NULL"), (dict(voxels=None), "NULL"), (dict(ws=None), "NULL")):
        refused(vox(**kw), word)
    for B, G, word in ((0, 8, "B=0"), (1, 1, "G=1"), (1, 257, "G=257")):
        refused(lib.cnerf_voxelize_bytes(B, G, ctypes.byref(nb)), word)

    rays = L.Rays()
    rays.origins = rays.dirs = 0x1000

    def hit(B=2, P=10, rays=rays, voxels=fake, G=8, lo=(-0.6, -0.6, -0.6), side=1.2, layout=0, t_min=0.2, t_max=2.0, S=16, bg=(1.0, 1.0, 1.0), pixels=fake):
        return lib.cnerf_voxel_first_hit(B, P, None if rays is None else ctypes.byref(rays), voxels, G, f3(lo), side, layout, t_min, t_max, S, f3(bg), pixels,
                                         None, None, None)

    no_origins, no_dirs = L.Rays(), L.Rays()
    no_origins.dirs = no_dirs.origins = 0x1000
    for kw, word in ((dict(B=0), "B=0"), (dict(P=0), "rays_per_image=0"), (dict(G=1), "G=1"), (dict(G=300), "G=300"), (dict(side=0.0), "side"),
                     (dict(side=nan), "side"), (dict(side=1e-45), "not finite"), (dict(lo=(0.0, nan, 0.0)), "lo[1]"), (dict(layout=3), "layout=3"), (dict(S=1), "S=1"), (dict(S=1025), "S=1025"),
                     (dict(t_min=1.0, t_max=1.0), "t_max"), (dict(t_min=2.0, t_max=1.0), "t_max"), (dict(t_min=nan), "finite"), (dict(t_max=inf), "finite"),
                     (dict(t_min=-inf), "finite"), (dict(rays=None), "NULL"), (dict(rays=no_origins), "NULL"), (dict(rays=no_dirs), "NULL"),
                     (dict(voxels=None), "NULL"), (dict(bg=None), "NULL"), (dict(pixels=None), "NULL"), (dict(lo=None), "lo")):
        refused(hit(**kw), word)


# ---------------------------------------------------------------------------------------------------------------------
# the oracles against the reference's arithmetic in float64
# ---------------------------------------------------------------------------------------------------------------------
def test_voxelize32_equals_the_open3d_rule_in_float64():
    """3 x 20,000 uniform points at G = 64, some beyond the cube so that the clip acts.  A point whose float64 cell coordinate lies within
    2^-21 G of an integer on some axis may fall either way in float32 and is left out (expected share 3 axes x 2 x 2^-21 x 64 / 1 per
    unit = 1.8e-4; at most 0.1 %).  Counts then agree exactly; colours within 2^-24: the quantisation moves an addend by at most 2^-25,
    so the mean by as much, and the final float32 rounding of a value <= 1 adds at most 2^-25."""
    G, length = 64, 1.2
    rng = np.random.default_rng(5)
    worst = 0.0
    for b in range(3):
        pts = np.concatenate([rng.uniform(-0.62, 0.62, (20000, 3)), rng.uniform(-0.1, 1.1, (20000, 3))], 1).astype(F)
        t = VC.open3d_t64(pts[:, :3], G, length)
        near = (np.abs(t - np.rint(t)) < 2.0 ** -21 * G).any(1)
        assert near.mean() <= 1e-3
        kept = pts[~near]
        assert (np.abs(kept[:, :3]) > 0.6).any() and (kept[:, 3:] < 0).any() and (kept[:, 3:] > 1).any()
        vox, cnt = VC.voxelize32(kept[None], G, -length / 2, length, clip_margin=1e-4, layout=1)
        c64, col64 = VC.open3d_f64(kept, G, length)
        assert cnt.sum() == len(kept) and np.array_equal(cnt[0], c64)
        assert np.array_equal(vox[0, ..., 0], (c64 > 0).astype(F)) and c64.max() >= 2
        err = np.abs(vox[0, ..., 1:].astype(np.float64) - col64).max()
        worst = max(worst, err)
        print(f"image {b}: left out {near.sum()} points, max colour error {err:.3g} (gate {2.0 ** -24:.3g})")
        assert err <= 2.0 ** -24
        enc, cnt0 = VC.voxelize32(kept[None], G, -length / 2, length, clip_margin=1e-4, layout=0)       # the other layout: a transpose
        assert np.array_equal(enc[0], vox[0].transpose(3, 2, 1, 0)) and np.array_equal(cnt0[0], cnt[0].transpose(2, 1, 0))
    assert worst > 0


def first_hit_scene():
    """G = 16, S = 32: a tenth of the cells occupied, 3000 rays between two points of [-0.5, 0.5]^3, t in [0, 1]: every sample is inside."""
    G, S, length = 16, 32, 1.2
    rng = np.random.default_rng(6)
    vox = np.zeros((2, G, G, G, 4), F)
    vox[..., 0] = rng.uniform(size=(2, G, G, G)) < 0.1
    vox[..., 1:] = rng.uniform(size=(2, G, G, G, 3)) * vox[..., :1]
    o = rng.uniform(-0.5, 0.5, (2, 1500, 3)).astype(F)
    e = rng.uniform(-0.5, 0.5, (2, 1500, 3)).astype(F)
    return vox, o, (e - o).astype(F), G, S, length


def test_first_hit32_equals_voxel_interpolate_in_float64():
    """Rays with a sample whose float64 cell coordinate lies within 2^-21 G of an integer are left out (expected share 32 samples x 3 axes
    x 2 x 2^-21 G per cell = 0.15 %; cap 1 %); on the others the pixels agree exactly."""
    vox, o, d, G, S, length = first_hit_scene()
    t64 = VC.interpolate_u64(o, d, length, G, 0.0, 1.0, S) + 0.5
    assert t64.min() > 0 and t64.max() < G                           # every sample inside the cube
    near = (np.abs(t64 - np.rint(t64)) < 2.0 ** -21 * G).any((-1, -2))
    print(f"rays left out: {near.sum()} of {near.size} ({near.mean():.3%})")
    assert near.mean() <= 0.01
    want = VC.interpolate_f64(vox, o, d, length, 0.0, 1.0, S, layout=1)
    pixels, hit_t, hit_cell = VC.first_hit32(vox, o, d, -length / 2, length, 0.0, 1.0, S, layout=1)
    assert np.array_equal(pixels[~near], want[~near])
    hit = hit_cell >= 0
    assert 0.2 < hit.mean() < 0.98 and np.isinf(hit_t[~hit]).all() and (pixels[~hit] == 1).all()
    ts = VC.linspace32(0.0, 1.0, S)
    assert np.isin(hit_t[hit], ts).all()
    enc = np.ascontiguousarray(vox.transpose(0, 4, 3, 2, 1))         # the encoder's layout gives the same picture
    again = VC.first_hit32(enc, o, d, -length / 2, length, 0.0, 1.0, S, layout=0)
    assert all(np.array_equal(a, b) for a, b in zip(again, (pixels, hit_t, hit_cell)))
