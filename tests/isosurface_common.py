"""Marching tetrahedra on the Kuhn split, restated in vectorised NumPy float32: the oracle of cnerf_isosurface_* (include/cnerf.h states
the algorithm).  The oracle itself is checked by geometry only (tests/test_isosurface_cpu.py): planes, balls, a torus.

    vertices, faces, vertex_attrs = isosurface(values, level, lo, pitch, attrs)

and the helpers the geometric checks share: canonical faces, the directed-edge census, signed volume, Euler characteristic."""
import itertools

import numpy as np

F = np.float32
PERMUTATIONS = sorted(itertools.permutations(range(3)))          # tetrahedron t belongs to PERMUTATIONS[t] = (a, b, c)
PARITY = [0, 1, 1, 0, 0, 1]                                      # of the permutation

# FLIP[t][case]: exchange the last two indices of the case's triangles (case bit x = INSIDE of w_x); rows of equal parity are equal
FLIP = np.array([
    [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
    [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0],
    [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0],
    [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
    [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0],
    [0, 1, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0],
], np.uint8)


def tet_corners(t):
    """Corner offsets of w0..w3 as numbers d0 + 2 d1 + 4 d2."""
    a, b, _ = PERMUTATIONS[t]
    return [0, 1 << a, (1 << a) | (1 << b), 7]


def offset(j):
    return (j & 1, (j >> 1) & 1, (j >> 2) & 1)


def case_triangles(case):
    """Triangles of a 4-bit case before orientation: a list of triples of tetrahedron edges (x, y)."""
    ins = [x for x in range(4) if (case >> x) & 1]
    out = [x for x in range(4) if not (case >> x) & 1]
    if not ins or not out:
        return []
    if len(ins) == 1 or len(out) == 1:
        m = ins[0] if len(ins) == 1 else out[0]
        p, q, r = [x for x in range(4) if x != m]
        return [[(m, p), (m, q), (m, r)]]
    (a, b), (c, d) = ins, out
    q = [(a, c), (a, d), (b, d), (b, c)]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def oriented_case_triangles(t, case):
    return [[tri[0], tri[2], tri[1]] if FLIP[t][case] else tri for tri in case_triangles(case)]


def count_table():
    """Triangles of a cell by its 8-bit code (bit j = INSIDE of the corner with offset number j)."""
    out = np.zeros(256, np.uint8)
    for code in range(256):
        for t in range(6):
            case = sum(((code >> w) & 1) << x for x, w in enumerate(tet_corners(t)))
            out[code] += len(case_triangles(case))
    return out


def positions(shape, lo, pitch):
    """(N0,N1,N2,3) float32: component c of point i = (float)i_c * pitch + lo_c, the product rounded, then the sum."""
    axes = [(np.arange(n).astype(F) * F(pitch)).astype(F) + F(l) for n, l in zip(shape, lo)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(F)


def crossing_edges(inside):
    """Lattice edges whose ends differ in INSIDE, in vertex order (owner's flat index ascending, kind ascending) -> cross (n,7) bool
    (cross[p, k]: the edge of kind k + 1 owned by point p), and per vertex the flat indices of its owner and of the other end."""
    n = inside.size
    flat = np.arange(n).reshape(inside.shape)
    cross = np.zeros((n, 7), bool)
    far = np.zeros((n, 7), np.int64)
    for j in range(1, 8):
        d = offset(j)
        own = tuple(slice(0, s - dd) for s, dd in zip(inside.shape, d))
        oth = tuple(slice(dd, s) for s, dd in zip(inside.shape, d))
        cross[flat[own].ravel(), j - 1] = (inside[own] != inside[oth]).ravel()
        far[flat[own].ravel(), j - 1] = flat[oth].ravel()
    owner, kind = np.nonzero(cross)                              # row-major: owner ascending, kind ascending
    return cross, owner, far[owner, kind]


def is_inside(values, level):
    with np.errstate(invalid="ignore"):
        return np.asarray(values, F) > F(level)                  # False for a NaN and for a value equal to the level


def isosurface(values, level, lo=(0.0, 0.0, 0.0), pitch=1.0, attrs=None):
    """-> vertices (Nv,3) float32, faces (Nt,3) int32, vertex_attrs (Nv,C) float32 or None."""
    v = np.ascontiguousarray(values, F)
    N0, N1, N2 = v.shape
    n = v.size
    level = F(level)
    inside = is_inside(v, level)
    flat = np.arange(n).reshape(v.shape)
    pos = positions(v.shape, lo, pitch)
    cross, owner, other = crossing_edges(inside)
    vid = (np.cumsum(cross.ravel()) - 1).reshape(n, 7)           # valid where cross
    v0, v1 = v.ravel()[owner], v.ravel()[other]
    with np.errstate(all="ignore"):
        t = ((level - v0).astype(F) / (v1 - v0).astype(F)).astype(F)
        t = np.where(np.isfinite(v0) & np.isfinite(v1), t, F(0.5)).astype(F)
        P0, P1 = pos.reshape(n, 3)[owner], pos.reshape(n, 3)[other]
        vertices = (P0 + (t[:, None] * (P1 - P0).astype(F)).astype(F)).astype(F)
        vattrs = None
        if attrs is not None:
            A = np.ascontiguousarray(attrs, F).reshape(n, -1)
            a0, a1 = A[owner], A[other]
            vattrs = (a0 + (t[:, None] * (a1 - a0).astype(F)).astype(F)).astype(F)
    # triangles: (cell, tetrahedron, triangle) in that order
    cells = flat[:-1, :-1, :-1].ravel()                          # owner point of every cell, in cell flat order
    step = lambda j: (j & 1) * N1 * N2 + ((j >> 1) & 1) * N2 + ((j >> 2) & 1)
    ins = inside.ravel()
    tri = np.full((cells.size, 6, 2, 3), -1, np.int64)
    for t_ in range(6):
        w = tet_corners(t_)
        case = sum(ins[cells + step(w[x])].astype(np.int64) << x for x in range(4))
        for c in range(1, 15):
            sel = np.nonzero(case == c)[0]
            if not sel.size:
                continue
            for k, edges in enumerate(oriented_case_triangles(t_, c)):
                for i, (x, y) in enumerate(edges):
                    l, h = min(x, y), max(x, y)
                    tri[sel, t_, k, i] = vid[cells[sel] + step(w[l]), (w[h] ^ w[l]) - 1]
    tri = tri.reshape(-1, 3)
    faces = tri[tri[:, 0] >= 0].astype(np.int32)
    return vertices, faces, vattrs


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the geometric checks
# ---------------------------------------------------------------------------------------------------------------------
def canonical_faces(faces):
    """Each triple rotated so that its smallest index leads: the orientation is kept."""
    f = np.asarray(faces)
    k = np.argmin(f, 1)
    r = np.arange(len(f))
    return np.stack([f[r, k], f[r, (k + 1) % 3], f[r, (k + 2) % 3]], 1)


def directed_edges(faces):
    """(3 Nt, 2): the directed edges of every face."""
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def edge_census(faces):
    """-> (largest number of times one directed edge occurs, number of directed edges whose reverse does not occur exactly once)."""
    e = directed_edges(faces)
    key = e[:, 0] * (e.max() + 1) + e[:, 1]
    rev = e[:, 1] * (e.max() + 1) + e[:, 0]
    keys, counts = np.unique(key, return_counts=True)
    return int(counts.max()), int((~np.isin(rev, keys)).sum() + (counts != 1).sum())


def signed_volume(vertices, faces):
    """Volume enclosed by a closed mesh whose normals point outward (float64)."""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def normals(vertices, faces):
    """Right-hand normals (float64), their length twice the area."""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def euler_characteristic(n_vertices, faces):
    e = np.sort(directed_edges(faces), 1)
    return int(n_vertices - len(np.unique(e, axis=0)) + len(faces))


def ulp_tolerance(reference, ulps=2):
    """`ulps` units in the last place of the largest magnitude in `reference` (float32)."""
    m = F(np.max(np.abs(reference))) if np.size(reference) else F(0)
    return float(ulps * np.spacing(m))


def read_ply(path):
    """-> header lines, the vertex records and the face records of a binary little-endian PLY as write_ply lays it out."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").split("\n")
    nv = int(next(h for h in header if h.startswith("element vertex")).split()[-1])
    nf = int(next(h for h in header if h.startswith("element face")).split()[-1])
    colored = "property uchar red" in header
    vdt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if colored else [])
    vert = np.frombuffer(raw, np.dtype(vdt), nv, end)
    face = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<i4", (3,))]), nf, end + vert.nbytes)
    assert end + vert.nbytes + face.nbytes == len(raw)
    return header, vert, face


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
def ball_field(shape, centers, radius, lo=(0.0, 0.0, 0.0), pitch=1.0):
    """max over the balls of r^2 - |x - c|^2 at the lattice points (float32 values of a float64 evaluation)."""
    x = positions(shape, lo, pitch).astype(np.float64)
    return np.max([radius ** 2 - ((x - np.asarray(c, np.float64)) ** 2).sum(-1) for c in centers], 0).astype(F)


def torus_field(shape, center, R, r, lo=(0.0, 0.0, 0.0), pitch=1.0):
    """r^2 - (sqrt(x^2 + y^2) - R)^2 - z^2 about `center`, the axis along lattice axis 2."""
    x = positions(shape, lo, pitch).astype(np.float64) - np.asarray(center, np.float64)
    return (r ** 2 - (np.hypot(x[..., 0], x[..., 1]) - R) ** 2 - x[..., 2] ** 2).astype(F)


def plane_field(shape, nrm, c, lo=(0.0, 0.0, 0.0), pitch=1.0):
    x = positions(shape, lo, pitch).astype(np.float64)
    return (x @ np.asarray(nrm, np.float64) + c).astype(F)
