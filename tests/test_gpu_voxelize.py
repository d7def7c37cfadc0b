"""Voxel grids of point clouds on the GPU: cnerf_voxelize and cnerf_voxel_first_hit (through ops and through ctypes alone) against their
NumPy statements (tests/voxelize_common.py), bit for bit on every output; then voxels.py and the trainer's voxelize_pcl switch end to end.
Every case is a few hundred to a few ten thousand points or rays, but for the one that outgrows the launch grid (540,000 of each)."""
import ctypes as C

import numpy as np
import pytest
import torch

import voxelize_common as VC

pytestmark = pytest.mark.gpu

F = np.float32
LO, SIDE = (-0.6, -0.6, -0.6), 1.2
SENTINEL_V, SENTINEL_C = 12345.0, -77
LAYOUT_NAME = {0: "encoder", 1: "npz"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def gpu_voxelize(dev, pts, G, lo=LO, side=SIDE, lengths=None, clip=1e-4, layout=0):
    from cnerf_amd import ops
    v, c = ops.voxelize(on(dev, pts, F), G, lo, side, lengths=on(dev, lengths, np.int32), clip_margin=clip, layout=LAYOUT_NAME[layout], want_counts=True)
    assert v.dtype == torch.float32 and c.dtype == torch.int32 and v.is_cuda and not v.requires_grad
    return v.cpu().numpy(), c.cpu().numpy()


def raw_voxelize(dev, pts, G, lo=LO, side=SIDE, lengths=None, clip=1e-4, layout=0):
    """The entry through ctypes with a caller-made workspace (filled with garbage) and outputs pre-filled with a sentinel."""
    from cnerf_amd import ops, _lib as L
    lib = L.lib()
    B, n, stride = pts.shape
    pd, ld = on(dev, pts, F), on(dev, lengths, np.int32)
    nb = C.c_size_t(0)
    L.check(lib.cnerf_voxelize_bytes(B, G, C.byref(nb)), "bytes")
    ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device=dev)
    v = torch.full((B, 4, G, G, G) if layout == 0 else (B, G, G, G, 4), SENTINEL_V, dtype=torch.float32, device=dev)
    c = torch.full((B, G, G, G), SENTINEL_C, dtype=torch.int32, device=dev)
    L.check(lib.cnerf_voxelize(B, n, stride, L.ptr(pd), L.ptr(ld), G, (C.c_float * 3)(*lo), side, -1.0 if clip is None else clip, layout, L.ptr(v), L.ptr(c),
                               L.ptr(ws), ops._stream()), "voxelize")
    return v.cpu().numpy(), c.cpu().numpy()


def assert_same(got, want, what):
    assert VC.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), what


def edge_cloud(G, lo, side, stride=6, seed=0):
    """One cloud with every edge of the contract: random points, 300 points of colour 1.0 in one cell (their sum 300 x 2^24 passes 2^32),
    points exactly on cell faces and on the cube's faces, -0.0 and 0.0 coordinates, points beyond the cube (near, far, infinite), NaN
    coordinates, colours below 0, above 1 and NaN."""
    rng = np.random.default_rng(seed)
    lo3 = np.asarray(lo, F)
    cell = F(F(side) / F(G))
    inside = (lo3 + rng.uniform(0.02, 0.98, (500, 3)) * side).astype(F)
    one_cell = (lo3 + (np.asarray([G - 1, 0, G // 2]) + rng.uniform(0.1, 0.9, (300, 3))) * cell).astype(F)
    planes = (lo3[None] + (np.arange(G + 1, dtype=F)[:, None] * cell).astype(F)).astype(F)               # (G+1, 3): every cell face
    faces = np.concatenate([np.stack([planes[:, 0], inside[:G + 1, 1], inside[:G + 1, 2]], 1), np.stack([inside[:G + 1, 0], planes[:, 1], planes[:, 2]], 1),
                            planes, (lo3 + F(side)).astype(F)[None].repeat(2, 0), lo3[None]])
    zeros = np.asarray([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.1], [-0.0, -0.0, -0.0]], F)
    outside = np.asarray([[lo3[0] - 0.1, 0, 0], [0, lo3[1] + side + 0.1, 0], [0, 0, 1e30], [-1e30, 0, 0], [np.inf, 0, 0], [0, -np.inf, 0], [np.inf, np.inf, -np.inf],
                          [3e38, -3e38, 3e38]], F)
    nans = np.asarray([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.nan, np.nan, np.nan], [np.nan, np.inf, 0]], F)
    xyz = np.concatenate([inside, one_cell, faces, zeros, outside, nans]).astype(F)
    rgb = rng.uniform(0, 1, (len(xyz), 3)).astype(F)
    rgb[500:800] = 1.0
    rgb[:40] = rng.uniform(-0.5, 1.5, (40, 3))
    rgb[40:46] = np.asarray([[np.nan, 0.5, 0.5], [0.5, np.nan, 2.0], [-np.inf, np.inf, np.nan], [-0.0, 1.0, 0.0], [1e-9, 1 - 1e-9, 0.5], [2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -25]], F)
    rows = np.concatenate([xyz, rgb, rng.uniform(-9, 9, (len(xyz), stride - 6)).astype(F)], 1)
    return rows[rng.permutation(len(rows))], len(nans)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the voxeliser against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("G", (2, 5, 64))
def test_every_edge_of_the_contract(dev, G, layout):
    for lo in (LO, (0.0, -0.3, -1.0)):                   # the second cube has a face at x = 0: -0.0 lies on it
        pts, n_nan = edge_cloud(G, lo, SIDE, seed=G)
        pts = pts[None]
        for clip in (1e-4, 0.0, None):
            want = VC.voxelize32(pts, G, lo, SIDE, clip_margin=clip, layout=layout)
            v, c = raw_voxelize(dev, pts, G, lo, SIDE, clip=clip, layout=layout)
            assert (v != SENTINEL_V).all() and (c != SENTINEL_C).all(), (lo, clip)      # every element is written
            assert_same((v, c), want, (lo, clip, "ctypes"))
            again = gpu_voxelize(dev, pts, G, lo, SIDE, clip=clip, layout=layout)
            assert_same(again, want, (lo, clip, "ops"))
            assert_same(gpu_voxelize(dev, pts, G, lo, SIDE, clip=clip, layout=layout), again, "two runs")
            keep, _ = VC.cells32(pts[0, :, :3], G, lo, SIDE, clip)
            assert c.sum() == keep.sum()                                                # counts summed = the points not skipped
            if clip is None:
                assert c.sum() < pts.shape[1] - n_nan - 4                               # the points beyond the cube are skipped ...
            else:
                assert c.sum() == pts.shape[1] - n_nan                                  # ... or clipped into it: only a NaN position is skipped
            assert c.max() >= 300 and want[0].max() == 1.0 and ((want[0] > 0) & (want[0] < 1)).any()


@pytest.mark.parametrize("G", (2, 5, 64))
def test_one_point_and_wide_rows(dev, G):
    one = np.asarray([[[0.1, -0.2, 0.3, 0.25, 0.5, 0.75]]], F)
    for layout in (0, 1):
        want = VC.voxelize32(one, G, LO, SIDE, layout=layout)
        assert want[1].sum() == 1
        assert_same(raw_voxelize(dev, one, G, layout=layout), want, "n = 1")
    pts, _ = edge_cloud(G, LO, SIDE, stride=9, seed=3)
    assert pts.shape[1] == 9
    want = VC.voxelize32(pts[None], G, LO, SIDE, layout=0)
    assert_same(VC.voxelize32(pts[None, :, :6], G, LO, SIDE, layout=0), want, "the oracle reads six columns")
    assert_same(raw_voxelize(dev, pts[None], G, layout=0), want, "stride 9")
    assert_same(gpu_voxelize(dev, pts[None], G, layout=1), VC.voxelize32(pts[None], G, LO, SIDE, layout=1), "stride 9, npz")


@pytest.mark.parametrize("G", (2, 5, 64))
def test_seventy_thousand_points_in_one_cell(dev, G):
    """Contention: every add of the launch meets the same four words.  The mean of 70,000 colours is exact in the integer sums."""
    rng = np.random.default_rng(11)
    cell = SIDE / G
    xyz = (np.asarray(LO) + (np.asarray([1, G - 1, 0]) + rng.uniform(0.05, 0.95, (70000, 3))) * cell).astype(F)
    pts = np.concatenate([xyz, rng.uniform(0, 1, (70000, 3)).astype(F)], 1)[None]
    for layout in (0, 1):
        want = VC.voxelize32(pts, G, LO, SIDE, layout=layout)
        assert want[1].max() == 70000 and (want[1] > 0).sum() == 1
        assert_same(gpu_voxelize(dev, pts, G, layout=layout), want, layout)


@pytest.mark.parametrize("G", (2, 5, 64))
def test_lengths_are_read_on_the_device_and_clamped(dev, G):
    rng = np.random.default_rng(12)
    n = 700                                               # three blocks of points, the last one partial
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (3, n, 3)), rng.uniform(0, 1, (3, n, 3))], 2).astype(F)
    for lengths in ((0, n, 1), (-5, n + 9, 257), (n, 256, 255)):
        for layout in (0, 1):
            want = VC.voxelize32(pts, G, LO, SIDE, lengths=lengths, layout=layout)
            v, c = raw_voxelize(dev, pts, G, lengths=lengths, layout=layout)
            assert (v != SENTINEL_V).all() and (c != SENTINEL_C).all()
            assert_same((v, c), want, (lengths, layout))
            assert [int(c[b].sum()) for b in range(3)] == [min(max(k, 0), n) for k in lengths]
    assert_same(gpu_voxelize(dev, pts, G, lengths=(-5, n + 9, 257)), VC.voxelize32(pts, G, LO, SIDE, lengths=(0, n, 257)), "clamp")
    v, c = gpu_voxelize(dev, pts, G, lengths=(0, n, 1))
    assert not v[0].any() and not c[0].any() and c[2].sum() == 1


# The three kernels stride over their work with at most MAX_GRID blocks of BLOCK lanes (VOX_MAX_GRID, VOX_BLOCK of csrc/voxelize.hip): the
# cases below hand each of them more than that, so a block takes a second item -- "the same bits for every launch geometry".
MAX_GRID, BLOCK = 2048, 256


@pytest.mark.parametrize("layout", (0, 1))
def test_more_work_than_the_grid_has_lanes(dev, layout):
    rng = np.random.default_rng(14)
    B, n, G = 3, 180_000, 64
    assert B * -(-n // BLOCK) > MAX_GRID and B * G ** 3 > MAX_GRID * BLOCK       # accumulate: items of 256 rows; finish: cells
    pts = np.concatenate([rng.uniform(-0.62, 0.62, (B, n, 3)), rng.uniform(-0.1, 1.1, (B, n, 3))], 2).astype(F)
    lengths = (n, n - 77, 100_001)
    want = VC.voxelize32(pts, G, LO, SIDE, lengths=lengths, layout=layout)
    v, c = raw_voxelize(dev, pts, G, lengths=lengths, layout=layout)
    assert (v != SENTINEL_V).all() and (c != SENTINEL_C).all()
    assert_same((v, c), want, layout)
    assert [int(c[b].sum()) for b in range(B)] == list(lengths)
    P, S = 270_000, 3                                                             # first hit: one lane per ray
    assert 2 * P > MAX_GRID * BLOCK
    o, d = camera_rays(rng, 2, P)
    vox = grid(rng, 2, 5, 0.3, layout)
    want = VC.first_hit32(vox, o, d, LO, SIDE, 0.2, 2.0, S, layout=layout)
    got = raw_first_hit(dev, vox, o, d, S, layout)
    assert (got[0] != SENTINEL_V).all() and (got[2] != SENTINEL_C).all() and 0.05 < (want[2] >= 0).mean() < 0.95
    assert_same_hit(got, want, layout)


def test_ops_shapes_streams_and_refusals(dev):
    from cnerf_amd import ops, _lib as L
    rng = np.random.default_rng(13)
    pts = np.concatenate([rng.uniform(-0.6, 0.6, (2, 333, 3)), rng.uniform(0, 1, (2, 333, 3))], 2).astype(F)
    want = VC.voxelize32(pts, 5, LO, SIDE)
    pd = on(dev, pts, F)
    v1 = ops.voxelize(pd[1], 5, LO, SIDE)                 # (n,6): one image, no batch axis, no counts
    assert v1.shape == (4, 5, 5, 5) and VC.same_bits(v1.cpu().numpy(), want[0][1])
    v = ops.voxelize(pd, 5, -0.6, SIDE)                   # a number for lo
    assert VC.same_bits(v.cpu().numpy(), want[0])
    side_stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side_stream):
        v, c = ops.voxelize(pd, 5, LO, SIDE, want_counts=True)
    side_stream.synchronize()
    assert_same((v.cpu().numpy(), c.cpu().numpy()), want, "side stream")
    wide = torch.zeros(2, 333, 8, dtype=torch.float64, device=dev, requires_grad=True)      # a strided float64 view that requires grad
    with torch.no_grad():
        wide[..., :6] = pd
    v2 = ops.voxelize(wide[..., :6], 5, LO, SIDE)
    assert not v2.requires_grad and VC.same_bits(v2.cpu().numpy(), want[0])
    for bad in (pd[..., :5], pd.reshape(-1), pd[None]):
        with pytest.raises(L.CnerfError):
            ops.voxelize(bad, 5, LO, SIDE)
    for kw in (dict(layout="zyx"), dict(lengths=torch.tensor([1, 2, 3])), dict(clip_margin=0.7)):
        with pytest.raises(L.CnerfError):
            ops.voxelize(pd, 5, LO, SIDE, **kw)
    with pytest.raises(L.CnerfError):
        ops.voxelize(pd, 1, LO, SIDE)
    with pytest.raises(L.CnerfError):
        ops.voxelize(pd.cpu(), 5, LO, SIDE)               # no CPU fallback
    with pytest.raises(L.CnerfError):
        ops.voxel_first_hit(v.cpu(), pd[..., :3].cpu(), pd[..., 3:].cpu(), LO, SIDE, 0.0, 1.0, 8)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the first hit against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def gpu_first_hit(dev, vox, o, d, S, layout, t_min=0.2, t_max=2.0, bg=(1.0, 1.0, 1.0), lo=LO):
    from cnerf_amd import ops
    out = ops.voxel_first_hit(on(dev, vox, F), on(dev, o, F), on(dev, d, F), lo, SIDE, t_min, t_max, S, background=bg, layout=LAYOUT_NAME[layout])
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.float32 and out[2].dtype == torch.int32 and not out[0].requires_grad
    return tuple(x.cpu().numpy() for x in out)


def raw_first_hit(dev, vox, o, d, S, layout, t_min=0.2, t_max=2.0, bg=(1.0, 1.0, 1.0), lo=LO):
    from cnerf_amd import ops, _lib as L
    B, P = o.shape[:2]
    G = vox.shape[2]
    vd, od, dd = on(dev, vox, F), on(dev, o, F), on(dev, d, F)
    rays = L.Rays()
    rays.origins, rays.dirs = od.data_ptr(), dd.data_ptr()
    px = torch.full((B, P, 3), SENTINEL_V, dtype=torch.float32, device=dev)
    ht = torch.full((B, P), SENTINEL_V, dtype=torch.float32, device=dev)
    hc = torch.full((B, P), SENTINEL_C, dtype=torch.int32, device=dev)
    L.check(L.lib().cnerf_voxel_first_hit(B, P, C.byref(rays), L.ptr(vd), G, (C.c_float * 3)(*lo), SIDE, layout, t_min, t_max, S, (C.c_float * 3)(*bg),
                                          L.ptr(px), L.ptr(ht), L.ptr(hc), ops._stream()), "first_hit")
    only_pixels = torch.full((B, P, 3), SENTINEL_V, dtype=torch.float32, device=dev)      # the two optional outputs left out
    L.check(L.lib().cnerf_voxel_first_hit(B, P, C.byref(rays), L.ptr(vd), G, (C.c_float * 3)(*lo), SIDE, layout, t_min, t_max, S, (C.c_float * 3)(*bg),
                                          L.ptr(only_pixels), None, None, ops._stream()), "first_hit")
    assert torch.equal(only_pixels.view(torch.int32), px.view(torch.int32))
    return px.cpu().numpy(), ht.cpu().numpy(), hc.cpu().numpy()


def assert_same_hit(got, want, what):
    assert VC.same_bits(got[0], want[0]) and VC.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]), what


def grid(rng, B, G, share, layout):
    """[b, ix, iy, iz, ch] with `share` of the cells occupied, in the asked layout."""
    vox = np.zeros((B, G, G, G, 4), F)
    vox[..., 0] = rng.uniform(size=(B, G, G, G)) < share
    vox[..., 1:] = rng.uniform(size=(B, G, G, G, 3))          # empty cells carry colours too: they must not be seen
    return np.ascontiguousarray(vox.transpose(0, 4, 3, 2, 1)) if layout == 0 else vox


def camera_rays(rng, B, P):
    """Rays from a shell of radius 0.9-1.3 toward points of the cube, directions of length 0.5-1.5 (not normalised)."""
    o = rng.normal(size=(B, P, 3))
    o = o / np.linalg.norm(o, axis=-1, keepdims=True) * rng.uniform(0.9, 1.3, (B, P, 1))
    d = rng.uniform(-0.7, 0.7, (B, P, 3)) - o
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.5, 1.5, (B, P, 1))
    return o.astype(F), d.astype(F)


@pytest.mark.parametrize("layout", (0, 1))
@pytest.mark.parametrize("G", (2, 5, 64))
def test_first_hit_on_empty_full_and_sparse_grids(dev, G, layout):
    rng = np.random.default_rng(20 + G)
    o, d = camera_rays(rng, 2, 333)
    o[:, 0], d[:, 0] = (2.0, 2.0, 2.0), (1.0, 0.5, 0.25)                  # misses the cube
    o[:, 1], d[:, 1] = (0.1, 0.1, -2.0), (0.0, 0.0, 1.0)                  # two zero direction components, through the cube
    o[:, 2], d[:, 2] = (0.1, 2.0, 0.1), (0.0, 0.0, 1.0)                   # zero components, beside the cube
    o[:, 3], d[:, 3] = (0.05, -0.05, 0.05), (0.3, 0.2, -0.1)              # starts inside
    o[:, 4, 1] = np.nan                                                   # NaN rays
    d[:, 5, 2] = np.nan
    o[:, 6], d[:, 6] = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)                   # a ray that does not move: every sample in the middle cell
    o[:, 7, 0] = np.inf
    d[:, 8] = (-0.0, 0.0, -1.0)
    bg = (0.25, 1.0, -3.0)
    for share in (0.0, 1.0, 0.15):
        vox = grid(rng, 2, G, share, layout)
        for S in (2, 37, 1024):
            want = VC.first_hit32(vox, o, d, LO, SIDE, 0.2, 2.0, S, bg, layout)
            got = raw_first_hit(dev, vox, o, d, S, layout, bg=bg)
            assert (got[0] != SENTINEL_V).all() and (got[1] != SENTINEL_V).all() and (got[2] != SENTINEL_C).all()
            assert_same_hit(got, want, (share, S))
            assert_same_hit(gpu_first_hit(dev, vox, o, d, S, layout, bg=bg), want, (share, S, "ops"))
            hit = want[2] >= 0
            assert not hit[:, [0, 2, 4, 5, 7]].any() and np.isinf(want[1][~hit]).all() and (want[0][~hit] == np.asarray(bg, F)).all()
            assert np.isin(want[1][hit], VC.linspace32(0.2, 2.0, S)).all()         # hit_t is an element of the linspace
            if share == 0.0:
                assert not hit.any()
            if share == 1.0 and S >= 37:
                assert hit[:, [1, 3, 6]].all() and hit.mean() > 0.5
                assert (want[1][:, 3] == F(0.2)).all() and (want[1][:, 6] == F(0.2)).all()      # a start inside an occupied cell: the first sample


def test_first_hit_images_differ_and_nan_occupancy_counts(dev):
    rng = np.random.default_rng(31)
    G, S = 5, 64
    o, d = camera_rays(rng, 2, 500)
    for layout in (0, 1):
        vox = grid(rng, 2, G, 0.0, layout)
        xyzc = vox.transpose(0, 4, 3, 2, 1) if layout == 0 else vox       # a view: [b, ix, iy, iz, ch]
        xyzc[0, 2, 2, 2, 0] = np.nan                                      # image 0: one cell whose occupancy is NaN
        xyzc[1, 1, 3, 0, 0] = -2.5                                        # image 1: another cell, any non-zero value
        want = VC.first_hit32(vox, o, d, LO, SIDE, 0.2, 2.0, S, layout=layout)
        assert set(np.unique(want[2][0])) == {-1, (2 * G + 2) * G + 2} and set(np.unique(want[2][1])) == {-1, (1 * G + 3) * G + 0}
        assert_same_hit(gpu_first_hit(dev, vox, o, d, S, layout), want, layout)
        assert_same_hit(raw_first_hit(dev, vox, o, d, S, layout), want, layout)
    one = gpu_first_hit(dev, vox[1], o[1], d[1], S, 1)                    # a single grid with (P,3) rays: no batch axis
    assert one[0].shape == (500, 3) and one[2].shape == (500,) and VC.same_bits(one[0], want[0][1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. composed: voxels.py and the trainer
# ---------------------------------------------------------------------------------------------------------------------
def test_cloud_to_npz_round_trip(dev, tmp_path):
    from cnerf_amd import voxels as VX
    from cnerf_amd.training import formats
    rng = np.random.default_rng(40)
    pcl = np.concatenate([rng.uniform(-0.65, 0.65, (2, 3000, 3)), rng.uniform(0, 1, (2, 3000, 3))], 2).astype(F)
    vox = VX.voxelize_cloud(on(dev, pcl, F), resolution=32, length=1.2)
    assert vox.shape == (2, 4, 32, 32, 32) and not vox.requires_grad
    assert VC.same_bits(vox.cpu().numpy(), VC.voxelize32(pcl, 32, LO, SIDE, clip_margin=1e-4, layout=0)[0])
    path = str(tmp_path / "voxel_32.npz")
    VX.save_voxel_npz(path, vox[1], 1.2)
    with np.load(path) as f:
        assert set(f.files) == {"voxel", "length", "resolution", "noise_color", "noise_xyz"}
        assert f["voxel"].shape == (32, 32, 32, 4) and f["voxel"].dtype == np.float64 and int(f["resolution"]) == 32 and float(f["length"]) == 1.2
        assert VC.same_bits(f["voxel"], VC.voxelize32(pcl[1:], 32, LO, SIDE, clip_margin=1e-4, layout=1)[0][0])      # the order of voxel.npz
    back = formats.load_voxel_npz(path, resolution=32)
    assert torch.equal(back, vox[1].cpu())
    # the noise is drawn on the device from the given generator: the same seed, the same grid; another seed, another grid
    gen = lambda s: torch.Generator(device=dev).manual_seed(s)
    a = VX.voxelize_cloud(on(dev, pcl, F), 32, 1.2, noise_xyz=0.01, noise_color=0.02, generator=gen(1))
    b = VX.voxelize_cloud(on(dev, pcl, F), 32, 1.2, noise_xyz=0.01, noise_color=0.02, generator=gen(1))
    c = VX.voxelize_cloud(on(dev, pcl, F), 32, 1.2, noise_xyz=0.01, noise_color=0.02, generator=gen(2))
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, vox)
    assert int(a[:, 0].sum()) > 0 and float(a[:, 1:].min()) >= 0 and float(a[:, 1:].max()) <= 1


def test_surface_render_of_one_voxel(dev):
    from cnerf_amd import voxels as VX
    from cnerf_amd.generators.volumetric_rendering import pinhole_rays
    G, R, S, fov = 8, 24, 256, 49.134342641202636
    vox = np.zeros((2, 4, G, G, G), F)
    vox[0, :, 4, 3, 5] = (1.0, 0.25, 0.5, 0.75)                           # [ch, iz, iy, ix]
    vox[1, :, 2, 5, 3] = (1.0, 0.9, 0.1, 0.2)
    cams = np.tile(np.eye(4, dtype=F), (2, 1, 1))
    cams[:, 2, 3] = -1.0                                                  # on the -z axis, looking along +z
    cams[1, 0, 3] = 0.1
    cd = on(dev, cams, F)
    img = VX.voxel_surface_render(on(dev, vox, F), cd, R, fov, 0.2, 2.0, num_steps=S)
    assert img.shape == (2, 3, R, R) and img.dtype == torch.float32
    o, d = pinhole_rays(cd, R, fov)
    want, _, cell = VC.first_hit32(vox, o.cpu().numpy(), d.cpu().numpy(), LO, SIDE, 0.2, 2.0, S, layout=0)
    assert VC.same_bits(img.cpu().numpy(), want.reshape(2, R, R, 3).transpose(0, 3, 1, 2))
    lit = (cell >= 0).reshape(2, R, R)
    assert 4 <= lit[0].sum() < R * R // 4 and 4 <= lit[1].sum() < R * R // 4 and not np.array_equal(lit[0], lit[1])
    got = img.cpu().numpy()
    assert (got[0][:, lit[0]] == np.asarray([[0.25], [0.5], [0.75]], F)).all() and (got[0][:, ~lit[0]] == 1).all()


def test_trainer_voxelises_the_clouds_of_a_step(dev):
    import cnerf_amd  # noqa: F401
    from cnerf_amd.training import GanTrainer, default_metadata
    from cnerf_amd.training.gan_step import synthetic_sample
    torch.manual_seed(0)
    md = default_metadata(img_size=32, num_steps=12, batch_size=2, batch_split=1, hidden_dim=64)
    md["unet"].update(f_maps=8, num_levels=3)
    md["generator"]["z_dim"] = 32
    md["dataset"] = {"voxelize_pcl": True}
    md.update(voxel_resolution=32, noise_xyz=0.005, noise_color=0.01)
    with pytest.raises(ValueError):                       # the two cloud settings exclude each other
        GanTrainer({**md, "dataset": {"voxelize_pcl": True, "load_pcl": True}}, dev)
    tr = GanTrainer(md, dev)
    seen = []
    tr.encoder.register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone()))
    sample = synthetic_sample(2, 32, 32, dev, torch.Generator().manual_seed(1), pcl_points=2048)
    assert "voxel" not in sample and sample["pcl"].shape == (2, 2048, 6)
    enc_before = tr.encoder.final_conv.weight.detach().clone()
    tr.step(sample)
    torch.cuda.synchronize()
    assert seen and all(tuple(v.shape) == (2, 4, 32, 32, 32) for v in seen)
    occ = seen[0][:, 0]
    assert set(occ.unique().tolist()) == {0.0, 1.0} and 1500 < int(occ[0].sum()) <= 2048      # 2048 points in 32768 cells: few share one
    assert all(x == x and abs(x) < 1e4 for x in tr.losses["d"] + tr.losses["g"] + tr.losses["photo"])
    assert not torch.equal(tr.encoder.final_conv.weight, enc_before) and "voxel" not in sample
