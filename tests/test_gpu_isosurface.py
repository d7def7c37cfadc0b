"""Isosurfaces on the GPU: cnerf_isosurface_count / _emit (through ops.isosurface and through ctypes) against their NumPy statement
(tests/isosurface_common.py), geometry on the device's own output, and extract_shapes.extract_mesh end to end.

Shapes: one cell in all 256 corner patterns; 2 x 2 x 9 and 5 x 3 x 2 (less than a wave, thin on two axes), 9 x 8 x 7 (504 points: more than
one wave and more than one block), 33 x 17 x 13 (29 blocks, odd on every axis), 65 x 65 x 33 (545 blocks: more than SCAN_STEP, so the
block-sum scan carries from one round to the next).

Gates: counts, faces and their order exactly; vertices and attributes within 2 ulp of the largest coordinate (attribute) magnitude -- the
operation order is fixed and the division correctly rounded, so bit equality is expected (each comparison prints whether it held); the
gate stays at 2 ulp so that a compiler's choice of reciprocal does not fail a correct kernel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import isosurface_common as IC

pytestmark = pytest.mark.gpu

ISO_BLOCK = 256          # lattice points per block sum (csrc/cnerf_kernels.hpp)
SCAN_STEP = 256          # block sums the scan's one block takes per round (OCC_BLOCK in csrc/occupancy.hip): the scan's second level
LO, PITCH = (-0.6, 0.2, -1.3), 0.0371
SENTINEL = 12345.0
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def gpu_mesh(dev, values, level, lo=(0.0, 0.0, 0.0), pitch=1.0, attrs=None):
    from cnerf_amd import ops
    a = None if attrs is None else torch.from_numpy(np.ascontiguousarray(attrs, F)).to(dev)
    v, f, va = ops.isosurface(torch.from_numpy(np.ascontiguousarray(values, F)).to(dev), level, lo=lo, pitch=pitch, attrs=a)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda and v.dim() == 2 and f.dim() == 2
    return v.cpu().numpy(), f.cpu().numpy(), None if va is None else va.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_mesh_equals(got, want, what):
    """Counts, faces and face order exactly; vertices / attributes within 2 ulp of the largest magnitude (NaN == NaN)."""
    (gv, gf, ga), (wv, wf, wa) = got, want
    assert (len(gv), len(gf)) == (len(wv), len(wf)), what
    assert np.array_equal(IC.canonical_faces(gf), IC.canonical_faces(wf)) and np.array_equal(gf, wf), what
    for name, g, w in (("vertices", gv, wv), ("attributes", ga, wa)):
        if w is None:
            assert g is None
            continue
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), what
        tol = IC.ulp_tolerance(w[fin])
        err = float(np.abs(g[fin].astype(np.float64) - w[fin]).max()) if fin.any() else 0.0
        print(f"{what}: {name} max|err| {err:.3g} (gate {tol:.3g}), bit-identical: {same_bits(g, w)}")
        assert err <= tol, (what, name, err, tol)


def noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_one_cell_all_256_corner_patterns(dev):
    rng = np.random.default_rng(0)
    table = IC.count_table()
    for code in range(256):
        v = rng.uniform(0.1, 1.0, 8).astype(F)
        for j in range(8):
            if not (code >> j) & 1:
                v[j] = -v[j]
        # corner with offset number j = d0 + 2 d1 + 4 d2 sits at [d0, d1, d2]
        cell = np.zeros((2, 2, 2), F)
        for j in range(8):
            cell[IC.offset(j)] = v[j]
        want = IC.isosurface(cell, 0.0, LO, PITCH)
        assert len(want[1]) == table[code]
        assert_mesh_equals(gpu_mesh(dev, cell, 0.0, LO, PITCH), want, f"pattern {code}")


@pytest.mark.parametrize("shape", [(2, 2, 9), (5, 3, 2), (9, 8, 7), (33, 17, 13), (65, 65, 33)])
def test_noise_field_equals_the_oracle(dev, shape):
    if shape == (9, 8, 7):
        assert np.prod(shape) > ISO_BLOCK
    if shape == (65, 65, 33):
        assert -(-np.prod(shape) // ISO_BLOCK) > SCAN_STEP
    v = noise(shape, sum(shape))
    want = IC.isosurface(v, 0.1, LO, PITCH)
    assert len(want[1]) > np.prod(np.array(shape) - 1)           # a dense surface: more than a triangle per cell
    assert_mesh_equals(gpu_mesh(dev, v, 0.1, LO, PITCH), want, f"noise {shape}")


def test_two_runs_are_bit_identical(dev):
    v = noise((33, 17, 13), 5)
    attrs = noise((33, 17, 13, 3), 6)
    a, b = gpu_mesh(dev, v, 0.0, LO, PITCH, attrs), gpu_mesh(dev, v, 0.0, LO, PITCH, attrs)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and len(a[1]) > 0


def test_special_values(dev):
    """Corners equal to the level (outside), NaN (outside), +inf and -inf: the oracle's mesh; t = 0.5 on every edge with an end that is
    not finite; no NaN in a vertex whose edge has two finite ends."""
    shape = (9, 8, 7)
    rng = np.random.default_rng(3)
    v = noise(shape, 4)
    kind = rng.integers(0, 12, shape)
    level = F(0.25)
    v[kind == 0] = level
    v[kind == 1] = np.nan
    v[kind == 2] = np.inf
    v[kind == 3] = -np.inf
    pos = IC.positions(shape, LO, PITCH)
    want = IC.isosurface(v, level, LO, PITCH, attrs=pos)
    got = gpu_mesh(dev, v, level, LO, PITCH, attrs=pos)
    assert_mesh_equals(got, want, "special values")
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    # the t = 0.5 rule, seen in the device's vertices: the vertex of an edge with an end that is not finite is the edge's midpoint
    _, owner, other = IC.crossing_edges(IC.is_inside(v, level))
    bad = ~(np.isfinite(v.ravel()[owner]) & np.isfinite(v.ravel()[other]))
    P0, P1 = pos.reshape(-1, 3)[owner[bad]], pos.reshape(-1, 3)[other[bad]]
    assert bad.sum() > 20 and (~bad).sum() > 20 and (v == level).any() and np.isnan(v).any()
    assert np.abs(got[0][bad] - (P0 + F(0.5) * (P1 - P0))).max() <= IC.ulp_tolerance(pos)
    # equal to the level is outside: shifting those corners just below the level moves no face
    w = v.copy()
    w[v == level] = np.nextafter(level, F(-1))
    assert np.array_equal(gpu_mesh(dev, w, level, LO, PITCH)[1], got[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2. geometry on the device's own output
# ---------------------------------------------------------------------------------------------------------------------
def test_gpu_ball_is_closed_oriented_and_inside_the_ball(dev):
    r, c = 2.3, (4.1, 3.4, 2.9)
    verts, faces, _ = gpu_mesh(dev, IC.ball_field((9, 8, 7), [c], r), 0.0)
    assert IC.edge_census(faces) == (1, 0) and IC.euler_characteristic(len(verts), faces) == 2
    V, ball = IC.signed_volume(verts, faces), 4 / 3 * math.pi * r ** 3
    print("ball volume ratio", V / ball)
    assert 0 < V <= ball * (1 + 1e-5)


def test_gpu_two_balls_have_euler_characteristic_4(dev):
    verts, faces, _ = gpu_mesh(dev, IC.ball_field((12, 9, 8), [(2.6, 4.1, 3.4), (8.3, 3.8, 3.6)], 2.1), 0.0)
    assert IC.edge_census(faces) == (1, 0) and IC.euler_characteristic(len(verts), faces) == 4


def plane_bound(nrm, c, level, shape, lo, pitch):
    M = float(np.abs(IC.positions(shape, lo, pitch)).max())
    return 8 * 2.0 ** -24 * (np.abs(nrm).sum() * M + abs(c) + abs(level))


@pytest.mark.parametrize("nrm,c,level", [((1.0, 0.0, 0.0), 0.1, 0.25), ((0.3, -0.5, 0.8), 0.05, 0.0), ((-0.6, 0.2, 0.1), 0.3, 0.1)])
def test_gpu_plane(dev, nrm, c, level):
    shape, lo, pitch = (6, 5, 4), (-0.7, 0.3, -1.1), 0.37
    verts, faces, _ = gpu_mesh(dev, IC.plane_field(shape, nrm, c, lo, pitch), level, lo, pitch)
    resid = np.abs(verts.astype(np.float64) @ np.asarray(nrm) + c - level)
    assert len(faces) > 0 and resid.max() <= plane_bound(nrm, c, level, shape, lo, pitch)
    nn = IC.normals(verts, faces)
    area2 = np.linalg.norm(nn, axis=1)
    live = area2 > 1e-7
    assert live.any() and np.allclose(nn[live] / area2[live, None], -np.asarray(nrm) / np.linalg.norm(nrm), atol=1e-3)


def test_gpu_axis_plane_has_the_area_of_the_box_face(dev):
    shape, lo, pitch = (6, 5, 4), (-0.7, 0.3, -1.1), 0.37
    x = lo[1] + 2.4 * pitch
    verts, faces, _ = gpu_mesh(dev, IC.plane_field(shape, (0.0, 1.0, 0.0), -x, lo, pitch), 0.0, lo, pitch)
    want = (shape[0] - 1) * (shape[2] - 1) * pitch * pitch
    assert abs(np.linalg.norm(IC.normals(verts, faces), axis=1).sum() / 2 - want) <= 1e-5 * want


# ---------------------------------------------------------------------------------------------------------------------
# 3. attributes, empty surfaces, capacities
# ---------------------------------------------------------------------------------------------------------------------
def test_affine_attributes_follow_the_positions(dev):
    shape = (9, 8, 7)
    A = np.array([[0.3, -0.5, 0.8], [1.0, 0.0, 0.0], [-0.6, 0.2, 0.1], [0.0, 1.0, 1.0], [0.5, 0.5, -0.5]])
    b = np.array([0.05, 0.1, 0.3, -0.4, 0.0])
    pos = IC.positions(shape, LO, PITCH)
    attrs = (pos.astype(np.float64) @ A.T + b).astype(F)
    verts, faces, va = gpu_mesh(dev, noise(shape, 9), 0.0, LO, PITCH, attrs)
    assert va.shape == (len(verts), 5) and len(verts) > 0
    M = float(np.abs(pos).max())
    for k in range(5):
        resid = np.abs(verts.astype(np.float64) @ A[k] + b[k] - va[:, k])
        assert resid.max() <= 8 * 2.0 ** -24 * (np.abs(A[k]).sum() * M + abs(b[k])), k


def test_no_attributes_and_empty_surface(dev):
    from cnerf_amd import ops, _lib as L
    v = noise((5, 3, 2), 1)
    assert gpu_mesh(dev, v, 0.0)[2] is None
    for attrs in (None, np.zeros((5, 3, 2, 3), F)):
        verts, faces, va = gpu_mesh(dev, v, 100.0, attrs=attrs)      # all values below the level
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and (va is None if attrs is None else va.shape == (0, 3))
    with pytest.raises(L.CnerfError):
        ops.isosurface(torch.from_numpy(v), 0.0)                     # a CPU tensor


def test_capacities_cut_the_output_and_nothing_is_written_behind_them(dev):
    from cnerf_amd import ops, _lib as L
    lib = L.lib()
    shape = (33, 17, 13)
    v = noise(shape, 7)
    attrs = noise(shape + (2,), 8)
    full = gpu_mesh(dev, v, 0.0, LO, PITCH, attrs)
    nv, nt = len(full[0]), len(full[1])
    vals, att = torch.from_numpy(v).to(dev), torch.from_numpy(attrs).to(dev)
    nb = C.c_size_t(0)
    L.check(lib.cnerf_isosurface_bytes(*shape, C.byref(nb)), "bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    L.check(lib.cnerf_isosurface_count(*shape, L.ptr(vals), 0.0, L.ptr(counts), L.ptr(ws), ops._stream()), "count")
    assert counts.tolist() == [nv, nt]
    verts = torch.full((nv, 3), SENTINEL, device=dev)
    vattr = torch.full((nv, 2), SENTINEL, device=dev)
    tris = torch.full((nt, 3), -7, dtype=torch.int32, device=dev)
    cap_v, cap_t = nv // 2, nt // 2
    lo3 = (C.c_float * 3)(*LO)
    L.check(lib.cnerf_isosurface_emit(*shape, L.ptr(vals), 0.0, lo3, PITCH, L.ptr(att), 2, cap_v, cap_t, L.ptr(verts), L.ptr(vattr), L.ptr(tris),
                                      L.ptr(ws), ops._stream()), "emit")
    verts, vattr, tris = verts.cpu().numpy(), vattr.cpu().numpy(), tris.cpu().numpy()
    assert same_bits(verts[:cap_v], full[0][:cap_v]) and same_bits(vattr[:cap_v], full[2][:cap_v]) and np.array_equal(tris[:cap_t], full[1][:cap_t])
    assert (verts[cap_v:] == SENTINEL).all() and (vattr[cap_v:] == SENTINEL).all() and (tris[cap_t:] == -7).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_extract_mesh_end_to_end(dev, tmp_path):
    from cnerf_amd import extract_shapes as X
    from cnerf_amd.generators import ImplicitGenerator3d
    torch.manual_seed(11)
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 32, 32, 4, 64).to(dev)
    gen.set_device(dev)
    z = (torch.randn(1, 32, 8, 8, 8, device=dev), torch.randn(1, 32, device=dev))
    N = 16
    sigma = X.sample_generator(gen, z, voxel_resolution=N)
    level = float(np.median(sigma))
    pts, corner, pitch = X.create_samples(N, cube_length=1.2)
    with torch.no_grad():
        field = gen.siren(pts.to(dev), z, N, 1).reshape(N, N, N, 4).cpu().numpy()
    assert same_bits(field[..., 3], sigma)
    lo = (corner[2], corner[1], corner[0])
    want = IC.isosurface(sigma, level, lo, pitch, attrs=field[..., :3])
    v, f, c = X.extract_mesh(gen, z, voxel_resolution=N, level=level)
    assert v.is_cuda and f.is_cuda and c.is_cuda and len(want[1]) > 0
    assert_mesh_equals((v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()), want, "extract_mesh")
    v2, f2, c2 = X.extract_mesh(gen, z, voxel_resolution=N, level=level, colors=False, max_points=500)       # ragged chunks
    assert c2 is None and torch.equal(v2, v) and torch.equal(f2, f)
    path = str(tmp_path / "mesh.ply")
    X.write_ply(path, v, f, c)
    header, vert, face = IC.read_ply(path)
    assert f"element vertex {len(v)}" in header and f"element face {len(f)}" in header
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), v.cpu().numpy()) and np.array_equal(face["v"], f.cpu().numpy())
    rgb = (np.clip(c.cpu().numpy(), 0, 1) * F(255)).astype(np.uint8)
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), rgb)
