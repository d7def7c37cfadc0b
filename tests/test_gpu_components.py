"""Connected components of a lattice on the GPU: cnerf_components_label / _filter (through ops and through ctypes) against their NumPy
statement (tests/components_common.py), bit for bit -- labels, sizes, all four stats with status 0, the filtered lattice -- and the layers
above them end to end: ops.keep_components + ops.isosurface, extract_mesh, extract_mesh_tsdf.

Shapes: one cell in all 256 patterns (each neighbour kind and each non-kind alone); 3 x 3 x 3 (both directions of every kind at the interior
point); (5,7,67), (3,17,259), (2,2,1024), (1024,2,2) (rows that straddle waves and blocks, 9 to 52 blocks, thin on two axes either way);
one path of 4351 points that winds through 31 x 31 x 16 and its mirror image (the longest chains); 64^3 (1024 blocks, hundreds of
components).

The winding path: a path through EVERY point of a 16^3 lattice is the full lattice, which is one component by its own edges whatever the
path; so the 16 x 16 rows of 16 points are laid two apart in a 31 x 31 x 16 lattice and joined end to end by 255 single points (4351 points,
no shorter than the 4096 asked for), and the full 16^3 lattice (one component of 4096 points with root 0) is a case of its own."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_common as CC
import isosurface_common as IC
from test_gpu_isosurface import assert_mesh_equals

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(dev)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gpu_label(dev, v, level, invert=False, connectivity=14):
    from cnerf_amd import ops
    labels, sizes, stats = ops.connected_components(on(dev, v), level, invert=invert, connectivity=connectivity)
    assert labels.dtype == sizes.dtype == stats.dtype == torch.int32 and labels.is_cuda and sizes.is_cuda and stats.is_cuda
    assert tuple(labels.shape) == tuple(sizes.shape) == tuple(v.shape) and tuple(stats.shape) == (4,)
    return labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().numpy()


def assert_labels_equal(got, want, what):
    for name, g, w in zip(("labels", "sizes", "stats"), got, want):
        assert g.dtype == np.int32 and np.array_equal(g, w), (what, name, g.ravel()[:16], w.ravel()[:16])
    assert got[2][3] == 0, what


def check(dev, v, level, what, invert=False, connectivity=14):
    want = CC.label(v, level, invert, connectivity)
    assert_labels_equal(gpu_label(dev, v, level, invert, connectivity), want, (what, invert, connectivity))
    return want


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_one_cell_all_256_patterns(dev):
    """Two points of a cell are joined iff they differ by one of the kinds: every kind, and every non-kind such as (1,-1,0), alone."""
    n_components = {6: set(), 14: set()}
    for code in range(256):
        cell = np.full((2, 2, 2), -1.0, F)
        for j in range(8):
            if (code >> j) & 1:
                cell[IC.offset(j)] = 1.0
        for conn in (6, 14):
            for invert in (False, True):
                want = check(dev, cell, 0.0, f"pattern {code}", invert, conn)
                n_components[conn].add(int(want[2][0]))
    # the two corners (1,0,0), (0,1,0) differ by (1,-1,0): two components under 14 as under 6; (0,0,0), (1,1,0) differ by a kind
    anti, diag = np.full((2, 2, 2), -1.0, F), np.full((2, 2, 2), -1.0, F)
    anti[1, 0, 0] = anti[0, 1, 0] = diag[0, 0, 0] = diag[1, 1, 0] = 1.0
    assert gpu_label(dev, anti, 0.0)[2].tolist() == [2, 2, 1, 0] and gpu_label(dev, diag, 0.0)[2].tolist() == [1, 0, 2, 0]
    assert gpu_label(dev, diag, 0.0, connectivity=6)[2].tolist() == [2, 0, 1, 0]
    assert n_components[6] == {0, 1, 2, 3, 4} and n_components[14] == {0, 1, 2, 3}


def test_200_random_3x3x3_lattices(dev):
    rng = np.random.default_rng(1)
    for k in range(200):
        v = rng.standard_normal((3, 3, 3)).astype(F)
        v[1, 1, 1] = abs(v[1, 1, 1]) + 1                            # the interior point is selected: all its 14 (6) neighbours count
        check(dev, v, float(rng.uniform(-0.5, 0.8)), f"3x3x3 #{k}", invert=False, connectivity=(14, 6)[k % 2])
        check(dev, -v, float(rng.uniform(-0.8, 0.5)), f"3x3x3 #{k} inverted", invert=True, connectivity=(14, 6)[k // 2 % 2])


@pytest.mark.parametrize("shape", [(5, 7, 67), (3, 17, 259), (2, 2, 1024), (1024, 2, 2)])
def test_shapes_that_straddle_waves_and_blocks(dev, shape):
    rng = np.random.default_rng(sum(shape))
    assert np.prod(shape) > 4 * 256
    for density in (0.2, 0.5, 0.8):
        v = (rng.uniform(size=shape) < density).astype(F)
        for conn in (6, 14):
            want = check(dev, v, 0.5, f"{shape} density {density}", False, conn)
            assert want[2][0] >= (50 if density == 0.2 else 1)
        check(dev, v, 0.5, f"{shape} density {density}", True, 14)


def test_one_winding_path_and_its_mirror_image(dev):
    w = CC.winding_path()
    for conn in (14, 6):
        for name, v in (("path", w), ("mirrored path", np.ascontiguousarray(w[::-1, ::-1, ::-1]))):
            want = check(dev, v, 0.5, name, False, conn)
            assert want[2].tolist() == [1, int(np.nonzero(v.ravel())[0][0]), 4351, 0]
    assert np.nonzero(w.ravel())[0][0] == 0


def test_ties_empty_and_full(dev):
    # two components of equal size: the lowest root is the largest
    v = np.zeros((6, 5, 9), F)
    v[4, 1:3, 2:5] = 1
    v[1, 2:4, 5:8] = 1
    want = check(dev, v, 0.5, "tie")
    assert want[2].tolist() == [2, (1 * 5 + 2) * 9 + 5, 6, 0]
    for conn in (6, 14):
        got = gpu_label(dev, v, 2.0, connectivity=conn)            # nothing selected
        assert (got[0] == -1).all() and not got[1].any() and got[2].tolist() == [0, -1, 0, 0]
        want = check(dev, np.ones((16, 16, 16), F), 0.5, "full", False, conn)
        assert want[2].tolist() == [1, 0, 4096, 0] and not want[0].any()
    from cnerf_amd import ops
    x = on(dev, v)
    assert torch.equal(ops.keep_components(x, 2.0), x) and torch.equal(ops.keep_components(x, 2.0, largest=False, min_size=100), x)
    assert torch.equal(ops.keep_components(torch.ones(16, 16, 16, device=dev), 0.5), torch.ones(16, 16, 16, device=dev))
    # of the tie only the lower root is kept
    kept = ops.keep_components(x, 0.5, fill=-3.0).cpu().numpy()
    assert same_bits(kept, CC.keep(v, 0.5, fill=-3.0)) and (kept[1] >= 0).all() and (kept[4, 1:3, 2:5] == -3).all()


def test_special_values(dev):
    """Equal to the level and NaN are outside, so selected with invert; +inf is inside, -inf outside; -0.0 against level 0.0 is outside."""
    shape = (9, 8, 7)
    rng = np.random.default_rng(3)
    v = rng.standard_normal(shape).astype(F)
    kind = rng.integers(0, 10, shape)
    level = F(0.25)
    v[kind == 0] = level
    v[kind == 1] = np.nan
    v[kind == 2] = np.inf
    v[kind == 3] = -np.inf
    for invert in (False, True):
        for conn in (6, 14):
            want = check(dev, v, level, "special values", invert, conn)
            sel = want[0] >= 0
            assert sel[kind == 2].all() != invert and sel[(kind == 0) | (kind == 1) | (kind == 3)].all() == invert
    z = np.where(rng.uniform(size=shape) < 0.5, F(-0.0), F(0.0)).astype(F)
    z[kind >= 7] = np.nextafter(F(0), F(1))
    want = check(dev, z, 0.0, "signed zeros")
    assert np.array_equal(want[0] >= 0, kind >= 7)
    check(dev, z, 0.0, "signed zeros", True)
    from cnerf_amd import ops
    out = ops.keep_components(on(dev, v), float(level), fill=float(level)).cpu().numpy()      # a fill equal to the level is outside
    assert same_bits(out, CC.keep(v, level, fill=level))
    for kw in (dict(fill=0.3), dict(fill=0.2, invert=True), dict(fill=float(level), invert=True), dict(fill=float("nan"))):
        with pytest.raises(ValueError):
            ops.keep_components(on(dev, v), float(level), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the filter
# ---------------------------------------------------------------------------------------------------------------------
def test_filter_options_and_aliasing(dev):
    from cnerf_amd import _lib as L, ops
    shape = (9, 17, 35)
    v = np.random.default_rng(8).standard_normal(shape).astype(F)
    level = 0.7
    labels, sizes, stats = CC.label(v, level)
    assert stats[0] > 20 and stats[2] > 2 and (sizes == 1).any() and (sizes == 2).any()
    x = on(dev, v)
    cases = [dict(largest=True), dict(largest=True, min_size=int(stats[2])), dict(largest=True, min_size=int(stats[2]) + 1),
             dict(largest=False, min_size=0), dict(largest=False, min_size=1), dict(largest=False, min_size=2),
             dict(largest=False, min_size=int(stats[2])), dict(largest=False, min_size=int(stats[2]) + 1),
             dict(largest=False, min_size=3, fill=-7.5), dict(largest=True, connectivity=6), dict(largest=False, min_size=2, connectivity=6),
             dict(level=-0.7, largest=True, invert=True), dict(level=-0.7, largest=False, min_size=2, invert=True, fill=9.0)]
    n_changed = set()
    for kw in cases:
        kw = dict(kw)
        lv = kw.pop("level", level)
        got = ops.keep_components(x, lv, **kw)
        want = CC.keep(v, lv, **kw)
        assert got.data_ptr() != x.data_ptr() and same_bits(got.cpu().numpy(), want), kw
        n_changed.add(int((want != v).sum()))
    assert torch.equal(x, on(dev, v)) and len(n_changed) >= 9 and 0 in n_changed
    out, gl, gs, gst = ops.keep_components(x, level, min_size=2, return_labels=True)
    assert_labels_equal((gl.cpu().numpy(), gs.cpu().numpy(), gst.cpu().numpy()), (labels, sizes, stats), "return_labels")
    # out_values = values, through the C entry; the labels of before
    alias = x.clone()
    L.check(L.lib().cnerf_components_filter(*shape, L.ptr(alias), L.ptr(gl), L.ptr(gs), L.ptr(gst), 0, 2, -1.0, L.ptr(alias), ops._stream()), "filter")
    assert same_bits(alias.cpu().numpy(), CC.keep(v, level, largest=False, min_size=2, fill=-1.0))
    with pytest.raises(L.CnerfError):
        ops.connected_components(x, level, connectivity=26)
    with pytest.raises(L.CnerfError):
        ops.connected_components(x[0], level)
    with pytest.raises(L.CnerfError):
        ops.keep_components(torch.from_numpy(v), level)             # a CPU tensor


# ---------------------------------------------------------------------------------------------------------------------
# 3. a larger lattice: two runs, and the C entries alone on a second stream
# ---------------------------------------------------------------------------------------------------------------------
def test_64_cubed_noise_twice_and_through_ctypes_on_a_second_stream(dev):
    from cnerf_amd import _lib as L, ops
    lib = L.lib()
    N, level = 64, 1.0
    v = CC.smoothed_noise(N, 3)
    want = CC.label(v, level)
    assert 200 < want[2][0] < 1000
    want_kept = CC.keep(v, level, largest=False, min_size=50)
    x = on(dev, v)
    runs = []
    for _ in range(2):
        out, labels, sizes, stats = ops.keep_components(x, level, largest=False, min_size=50, return_labels=True)
        runs.append((labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().numpy(), out.cpu().numpy()))
    nb = C.c_size_t(0)
    L.check(lib.cnerf_components_bytes(N, N, N, C.byref(nb)), "bytes")
    stream = torch.cuda.Stream(device=dev)
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    labels = torch.full((N ** 3 + 64,), -7, dtype=torch.int32, device=dev)
    sizes = torch.full((N ** 3 + 64,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((4 + 64,), -7, dtype=torch.int32, device=dev)
    out = torch.full((N ** 3 + 64,), 12345.0, device=dev)
    torch.cuda.synchronize(dev)
    s = C.c_void_p(stream.cuda_stream)
    L.check(lib.cnerf_components_label(N, N, N, L.ptr(x), level, 0, 14, L.ptr(labels), L.ptr(sizes), L.ptr(stats), L.ptr(ws), s), "label")
    L.check(lib.cnerf_components_filter(N, N, N, L.ptr(x), L.ptr(labels), L.ptr(sizes), L.ptr(stats), 0, 50, float("-inf"), L.ptr(out), s), "filter")
    stream.synchronize()
    labels, sizes, stats, out = labels.cpu().numpy(), sizes.cpu().numpy(), stats.cpu().numpy(), out.cpu().numpy()
    assert (labels[N ** 3:] == -7).all() and (sizes[N ** 3:] == -7).all() and (stats[4:] == -7).all() and (out[N ** 3:] == 12345.0).all()
    runs.append((labels[:N ** 3].reshape(N, N, N), sizes[:N ** 3].reshape(N, N, N), stats[:4], out[:N ** 3].reshape(N, N, N)))
    for k, run in enumerate(runs):
        assert_labels_equal(run[:3], want, f"64^3 run {k}")
        assert same_bits(run[3], want_kept), k


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------
def euler(mesh):
    return IC.euler_characteristic(len(mesh[0]), mesh[1])


def host_mesh(mesh):
    return tuple(None if t is None else t.cpu().numpy() for t in mesh)


def test_ball_and_floaters_through_keep_components_and_isosurface(dev):
    from cnerf_amd import ops
    v, pitch = CC.ball_and_floaters(40, 40, 2, small=0.05)
    n_solids = int(CC.label(v, 0.0)[2][0])
    assert n_solids > 10
    x = on(dev, v)
    full = host_mesh(ops.isosurface(x, 0.0, pitch=pitch))
    kept = host_mesh(ops.isosurface(ops.keep_components(x, 0.0), 0.0, pitch=pitch))
    assert_mesh_equals(kept, IC.isosurface(CC.keep(v, 0.0), 0.0, (0.0, 0.0, 0.0), pitch), "ball and floaters")
    assert euler(full) == 2 * n_solids and euler(kept) == 2 and IC.edge_census(kept[1]) == (1, 0) and CC.is_submesh(kept, full)


class BlobGenerator:
    """Stands in for a generator in extract_mesh: sigma is positive in a ball and in three small ones, rgb is the position."""

    def __init__(self, device):
        self.device = device

    def siren(self, points, z, N, S):
        p = points.double()
        sig = 0.3 ** 2 - (p ** 2).sum(-1)
        for c, r in (((0.45, 0.4, -0.42), 0.09), ((-0.42, 0.45, 0.4), 0.07), ((0.4, -0.45, -0.4), 0.1)):
            sig = torch.maximum(sig, r ** 2 - ((p - torch.tensor(c, dtype=torch.float64, device=p.device)) ** 2).sum(-1))
        return torch.cat([points, sig.float().unsqueeze(-1)], -1)


def test_extract_mesh_keywords(dev):
    from cnerf_amd import extract_shapes as X
    from cnerf_amd.generators import ImplicitGenerator3d
    gen = BlobGenerator(dev)
    kw = dict(voxel_resolution=32, cube_length=1.2, level=0.0)
    plain, default = X.extract_mesh(gen, None, **kw), X.extract_mesh(gen, None, keep_largest=False, min_component=0, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, default))
    largest = X.extract_mesh(gen, None, keep_largest=True, **kw)
    by_size = X.extract_mesh(gen, None, min_component=500, **kw)
    assert euler(host_mesh(plain)) == 8 and euler(host_mesh(largest)) == 2 and all(torch.equal(a, b) for a, b in zip(largest, by_size))
    assert CC.is_submesh(host_mesh(largest), host_mesh(plain)) and largest[2].shape == (len(largest[0]), 3)
    assert euler(host_mesh(X.extract_mesh(gen, None, min_component=2, **kw))) == 8
    # a real generator: the filter runs on the lattice the isosurface reads (reversed columns and all), as the oracle chain says
    torch.manual_seed(11)
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 32, 32, 4, 64).to(dev)
    gen.set_device(dev)
    z = (torch.randn(1, 32, 8, 8, 8, device=dev), torch.randn(1, 32, device=dev))
    N = 16
    pts, corner, pitch = X.create_samples(N, cube_length=1.2)
    with torch.no_grad():
        field = gen.siren(pts.to(dev), z, N, 1).reshape(N, N, N, 4).cpu().numpy()
    level = float(np.quantile(field[..., 3], 0.8))
    lo = (corner[2], corner[1], corner[0])
    print("extract_mesh: solids at the 0.8 quantile:", CC.label(field[..., 3], level)[2][0])
    a, b = X.extract_mesh(gen, z, voxel_resolution=N, level=level), X.extract_mesh(gen, z, voxel_resolution=N, level=level, keep_largest=False)
    assert all(torch.equal(s, t) for s, t in zip(a, b))
    got = host_mesh(X.extract_mesh(gen, z, voxel_resolution=N, level=level, keep_largest=True))
    assert_mesh_equals(got, IC.isosurface(CC.keep(field[..., 3], level), level, lo, pitch, attrs=field[..., :3]), "extract_mesh keep_largest")
    assert 0 < len(got[1]) <= len(a[1]) and CC.is_submesh(got, host_mesh(a))


def test_extract_mesh_tsdf_keywords(dev):
    """The analytic ball of test_gpu_tsdf.py.  8 cameras and a cube twice the usual edge: voxels behind the ball that a view or two see are
    solid by the hidden rule and show as blobs at the cube's faces (7 solids at this size); keep_largest leaves the ball.  24 cameras
    without the hidden rule (hidden_min = 0): two nested spheres, Euler characteristic 4; fill_cavities leaves the outer one."""
    import reproject_common as RC
    from cnerf_amd import extract_shapes as X
    from test_gpu_tsdf import FOV, RAY_END, RAY_START, BallGenerator, N, R, SIDE
    gen = BallGenerator(dev)
    z = torch.zeros((1, 4), device=dev)
    args = (R, FOV, RAY_START, RAY_END, 12)
    cams8 = on(dev, RC.cameras(8, 5, 1.4, 1.6))
    kw = dict(voxel_resolution=N, cube_length=2 * SIDE)
    plain = X.extract_mesh_tsdf(gen, z, cams8, *args, **kw)
    default = X.extract_mesh_tsdf(gen, z, cams8, *args, keep_largest=False, min_component=0, fill_cavities=False, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, default))
    largest = X.extract_mesh_tsdf(gen, z, cams8, *args, keep_largest=True, **kw)
    assert euler(host_mesh(plain)) > 2 and euler(host_mesh(largest)) == 2 and IC.edge_census(host_mesh(largest)[1]) == (1, 0)
    assert CC.is_submesh(host_mesh(largest), host_mesh(plain)) and largest[2].shape == (len(largest[0]), 3)
    by_size = X.extract_mesh_tsdf(gen, z, cams8, *args, min_component=600, **kw)
    assert all(torch.equal(a, b) for a, b in zip(largest, by_size))
    # cavities
    cams24 = on(dev, RC.cameras(24, 5, 1.4, 1.6))
    kw = dict(voxel_resolution=N, cube_length=SIDE, hidden_min=0)
    nested = host_mesh(X.extract_mesh_tsdf(gen, z, cams24, *args, **kw))
    filled = host_mesh(X.extract_mesh_tsdf(gen, z, cams24, *args, fill_cavities=True, **kw))
    assert euler(nested) == 4 and euler(filled) == 2 and IC.edge_census(filled[1]) == (1, 0) and CC.is_submesh(filled, nested)
    assert all(np.array_equal(a, b) for a, b in zip(host_mesh(X.extract_mesh_tsdf(gen, z, cams24, *args, keep_largest=True, **kw)), nested))
    ruled = host_mesh(X.extract_mesh_tsdf(gen, z, cams24, *args, voxel_resolution=N, cube_length=SIDE))
    assert np.array_equal(filled[1], ruled[1])                      # the hidden rule's own answer: the same faces
