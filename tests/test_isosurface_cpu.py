"""Isosurfaces (cnerf_isosurface_*), no GPU: the host code's exports, workspace sizes and refusals; the orientation table against the
geometry; the NumPy statement of the algorithm (tests/isosurface_common.py) against planes, balls and a torus; write_ply."""
import ctypes
import math
import re

import numpy as np
import pytest

import isosurface_common as IC

ENTRIES = ("cnerf_isosurface_bytes", "cnerf_isosurface_count", "cnerf_isosurface_emit")
F = np.float32


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def test_exports_and_prototypes(L):
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10


def test_workspace_sizes_are_positive_and_grow_with_the_lattice(L):
    lib = L.lib()
    nb = ctypes.c_size_t()
    sizes = []
    for shape in ((2, 2, 2), (2, 2, 9), (9, 8, 7), (65, 65, 33), (256, 256, 256), (512, 512, 512)):
        assert lib.cnerf_isosurface_bytes(*shape, ctypes.byref(nb)) == 0, lib.cnerf_last_error()
        assert nb.value >= 9 * shape[0] * shape[1] * shape[2]      # a code byte and two int32 offsets per point
        sizes.append(nb.value)
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes[1:])) == len(sizes) - 1


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t()
    lo0 = (0.0, 0.0, 0.0)

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def count(shape=(8, 8, 8), values=fake, level=0.0, counts=fake, ws=fake):
        return lib.cnerf_isosurface_count(*shape, values, level, counts, ws, None)

    def emit(shape=(8, 8, 8), values=fake, level=0.0, lo=lo0, pitch=1.0, attrs=None, n_attr=0, max_v=10, max_t=10, vertices=fake, vattrs=None,
             triangles=fake, ws=fake):
        lo3 = (ctypes.c_float * 3)(*lo) if lo is not None else None
        return lib.cnerf_isosurface_emit(*shape, values, level, lo3, pitch, attrs, n_attr, max_v, max_t, vertices, vattrs, triangles, ws, None)

    for shape, word in (((1, 8, 8), "n0=1"), ((8, 0, 8), "n1=0"), ((8, 8, 1025), "n2=1025"), ((-3, 8, 8), "n0=-3"), ((1024, 1024, 256), "2^27")):
        refused(lib.cnerf_isosurface_bytes(*shape, ctypes.byref(nb)), word)
        refused(count(shape=shape), word)
        refused(emit(shape=shape), word)
    assert lib.cnerf_isosurface_bytes(1024, 1024, 128, ctypes.byref(nb)) == 0        # exactly 2^27 points
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(count(level=bad), "level")
        refused(emit(level=bad), "level")
        refused(emit(pitch=bad), "pitch")
        for c in range(3):
            lo = [0.0, 0.0, 0.0]
            lo[c] = bad
            refused(emit(lo=lo), f"lo[{c}]")
    for pitch in (0.0, -1.0):
        refused(emit(pitch=pitch), "pitch")
    refused(count(values=None), "NULL")
    refused(count(counts=None), "NULL")
    refused(count(ws=None), "NULL")
    for missing in ("values", "vertices", "triangles", "ws", "lo"):
        refused(emit(**{missing: None}), "NULL")
    for n_attr in (0, -1, 9):
        refused(emit(attrs=fake, vattrs=fake, n_attr=n_attr), f"n_attr={n_attr}")
    refused(emit(attrs=fake, n_attr=3), "vertex_attrs")
    refused(emit(vattrs=fake, n_attr=3), "vertex_attrs")
    refused(emit(max_v=-1), "max_vertices=-1")
    refused(emit(max_t=-5), "max_triangles=-5")


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
def test_orientation_table_against_the_geometry():
    """Vertices at the edge midpoints: every triangle's right-hand normal has a positive component along (centroid of the outside
    corners - centroid of the inside corners); cases 0 and 15 emit nothing; rows of equal parity are equal."""
    for t in range(6):
        w = [np.array(IC.offset(j), np.float64) for j in IC.tet_corners(t)]
        assert IC.oriented_case_triangles(t, 0) == [] and IC.oriented_case_triangles(t, 15) == []
        for case in range(1, 15):
            ins = [x for x in range(4) if (case >> x) & 1]
            out = [x for x in range(4) if not (case >> x) & 1]
            toward = np.mean([w[x] for x in out], 0) - np.mean([w[x] for x in ins], 0)
            tris = IC.oriented_case_triangles(t, case)
            assert len(tris) == (2 if len(ins) == 2 else 1)
            for tri in tris:
                p = [(w[x] + w[y]) / 2 for x, y in tri]
                assert np.cross(p[1] - p[0], p[2] - p[0]) @ toward > 1e-3, (t, case)
        assert np.array_equal(IC.FLIP[t], IC.FLIP[IC.PARITY[t]])              # rows 0 and 1 are the even and the odd one
    # the six tetrahedra tile the cell: volumes 1/6 each, alternating orientation by parity
    for t in range(6):
        w = [np.array(IC.offset(j), np.float64) for j in IC.tet_corners(t)]
        vol = np.linalg.det(np.stack([w[1] - w[0], w[2] - w[0], w[3] - w[0]])) / 6
        assert abs(vol - (1 / 6) * (1 - 2 * IC.PARITY[t])) < 1e-12


def test_count_table_is_the_sum_over_the_six_tetrahedra():
    table = IC.count_table()
    assert table[0] == 0 and table[255] == 0 and table.max() == 12 and table[1] == 6 and table[0x80] == 6        # both ends of the body diagonal
    for code in range(256):
        total = 0
        for t in range(6):
            case = sum(((code >> w) & 1) << x for x, w in enumerate(IC.tet_corners(t)))
            total += len(IC.oriented_case_triangles(t, case))
        assert table[code] == total
        assert table[code] == table[255 - code]


def test_kernel_source_holds_the_same_orientation_table(L):
    src = open(L.HERE + "/csrc/isosurface.hip").read()
    body = re.search(r"ISO_FLIP\[6\]\[16\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    rows = [[int(x) for x in re.findall(r"\d+", row)] for row in re.findall(r"\{([^{}]*)\}", body)]
    assert np.array_equal(np.array(rows, np.uint8), IC.FLIP)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on a plane
# ---------------------------------------------------------------------------------------------------------------------
PLANE_SHAPE, PLANE_LO, PLANE_PITCH = (6, 5, 4), (-0.7, 0.3, -1.1), 0.37


def plane_bound(nrm, c, level, shape=PLANE_SHAPE, lo=PLANE_LO, pitch=PLANE_PITCH):
    """8 * 2^-24 * (|n|_1 M + |c| + |level|), M the largest coordinate magnitude: the three roundings of t and of the position."""
    M = float(np.abs(IC.positions(shape, lo, pitch)).max())
    return 8 * 2.0 ** -24 * (np.abs(nrm).sum() * M + abs(c) + abs(level))


@pytest.mark.parametrize("nrm,c,level", [((1.0, 0.0, 0.0), 0.1, 0.25), ((0.3, -0.5, 0.8), 0.05, 0.0), ((-0.6, 0.2, 0.1), 0.3, 0.1), ((0.0, 1.0, 1.0), -0.4, 0.0)])
def test_oracle_on_a_plane(nrm, c, level):
    v = IC.plane_field(PLANE_SHAPE, nrm, c, PLANE_LO, PLANE_PITCH)
    verts, faces, _ = IC.isosurface(v, level, PLANE_LO, PLANE_PITCH)
    assert len(faces) > 0 and faces.min() == 0 and faces.max() == len(verts) - 1
    # the lattice values themselves are the plane's rounded to float32 (half an ulp of their size): within the bound's slack
    resid = np.abs(verts.astype(np.float64) @ np.asarray(nrm) + c - level)
    print("plane residual", resid.max(), "bound", plane_bound(nrm, c, level))
    assert resid.max() <= plane_bound(nrm, c, level)
    nn = IC.normals(verts, faces)
    area2 = np.linalg.norm(nn, axis=1)
    live = area2 > 1e-7
    unit = nn[live] / area2[live, None]
    assert live.any() and np.allclose(unit, -np.asarray(nrm) / np.linalg.norm(nrm), atol=1e-3)


def test_oracle_axis_plane_has_the_area_of_the_box_face():
    for axis in range(3):
        nrm = np.zeros(3)
        nrm[axis] = 1.0
        x = PLANE_LO[axis] + 2.4 * PLANE_PITCH                   # strictly between lattice planes 2 and 3
        v = IC.plane_field(PLANE_SHAPE, nrm, -x, PLANE_LO, PLANE_PITCH)
        verts, faces, _ = IC.isosurface(v, 0.0, PLANE_LO, PLANE_PITCH)
        other = [(PLANE_SHAPE[k] - 1) * PLANE_PITCH for k in range(3) if k != axis]
        area = np.linalg.norm(IC.normals(verts, faces), axis=1).sum() / 2
        assert abs(area - other[0] * other[1]) <= 1e-5 * other[0] * other[1]


# ---------------------------------------------------------------------------------------------------------------------
# the oracle on closed surfaces
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_ball_is_closed_oriented_and_inside_the_ball():
    r, c = 2.3, (4.1, 3.4, 2.9)
    verts, faces, _ = IC.isosurface(IC.ball_field((9, 8, 7), [c], r), 0.0)
    assert IC.edge_census(faces) == (1, 0)                       # every directed edge once, its reverse once
    assert IC.euler_characteristic(len(verts), faces) == 2
    V, ball = IC.signed_volume(verts, faces), 4 / 3 * math.pi * r ** 3
    print("ball volume ratio", V / ball)
    assert 0 < V <= ball * (1 + 1e-5)


def test_oracle_euler_characteristic_of_two_balls_and_a_torus():
    verts, faces, _ = IC.isosurface(IC.ball_field((12, 9, 8), [(2.6, 4.1, 3.4), (8.3, 3.8, 3.6)], 2.1), 0.0)
    assert IC.edge_census(faces) == (1, 0) and IC.euler_characteristic(len(verts), faces) == 4
    verts, faces, _ = IC.isosurface(IC.torus_field((24, 24, 12), (11.4, 11.6, 5.3), 7.0, 2.6), 0.0)
    assert IC.edge_census(faces) == (1, 0) and IC.euler_characteristic(len(verts), faces) == 0
    assert IC.signed_volume(verts, faces) > 0


def test_oracle_special_values_and_attributes():
    """A corner equal to the level is outside; t = 0.5 where an end is not finite; attributes follow the positions."""
    v = np.full((2, 2, 2), -1.0, F)
    v[0, 0, 0] = 3.0
    verts, faces, _ = IC.isosurface(v, 0.0)
    assert len(verts) == 7 and len(faces) == 6 and np.array_equal(verts[verts > 0], np.full(12, 0.75, F))
    v[1, 1, 1] = np.nan
    v[0, 0, 1] = -np.inf
    verts2, faces2, _ = IC.isosurface(v, 0.0)
    assert np.array_equal(faces2, faces) and np.isfinite(verts2).all()
    assert np.array_equal(verts2[3], [0, 0, 0.5]) and np.array_equal(verts2[6], [0.5, 0.5, 0.5])      # kinds 4 and 7: the edges to -inf and NaN
    assert np.array_equal(np.delete(verts2, [3, 6], 0), np.delete(verts, [3, 6], 0))
    v[...] = 0.0                                                 # every corner equal to the level: nothing is inside
    assert len(IC.isosurface(v, 0.0)[1]) == 0
    g = np.random.default_rng(0).standard_normal((5, 4, 3)).astype(F)
    pos = IC.positions(g.shape, (0.5, -1.0, 2.0), 0.25)
    verts, faces, va = IC.isosurface(g, 0.1, (0.5, -1.0, 2.0), 0.25, attrs=pos)
    assert va.shape == verts.shape and np.abs(va - verts).max() <= 4 * 2.0 ** -24 * np.abs(pos).max()


# ---------------------------------------------------------------------------------------------------------------------
# write_ply
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colored", [False, True])
def test_write_ply_round_trip(L, tmp_path, colored):
    from cnerf_amd import extract_shapes as X
    verts, faces, _ = IC.isosurface(IC.ball_field((6, 6, 6), [(2.4, 2.6, 2.5)], 1.7), 0.0)
    rgb = np.random.default_rng(1).uniform(-0.2, 1.2, (len(verts), 3)).astype(F) if colored else None
    path = str(tmp_path / "mesh.ply")
    X.write_ply(path, verts, faces, rgb)
    header, vert, face = IC.read_ply(path)
    assert header[:2] == ["ply", "format binary_little_endian 1.0"] and f"element vertex {len(verts)}" in header
    assert f"element face {len(faces)}" in header and "property list uchar int vertex_indices" in header
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), verts)
    assert (face["n"] == 3).all() and np.array_equal(face["v"], faces)
    if colored:
        want = (np.clip(rgb, 0, 1) * F(255)).astype(np.uint8)
        assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), want) and want.min() == 0 and want.max() == 255
    else:
        assert "red" not in vert.dtype.names
