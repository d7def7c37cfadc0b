"""Connected components of a scalar lattice, restated in vectorised NumPy: the oracle of cnerf_components_* (include/cnerf.h states the
contract).  Minimum-label propagation over the forward neighbour kinds, with pointer jumping, until nothing changes.

    labels, sizes, stats = label(values, level, invert=False, connectivity=14)
    out = keep(values, level, largest=True, min_size=0, fill=None, invert=False, connectivity=14)

The oracle itself is checked against scipy.ndimage.label where scipy is installed, and by geometry (tests/test_components_cpu.py).
Below it the lattices the CPU and GPU tests share."""
import numpy as np

import isosurface_common as IC

F = np.float32


def kinds(connectivity):
    """The forward offsets (d0,d1,d2): the seven Kuhn edge kinds for 14, the three axis kinds for 6."""
    if connectivity not in (6, 14):
        raise ValueError(f"connectivity={connectivity} must be 6 or 14")
    return [IC.offset(j) for j in range(1, 8) if connectivity == 14 or sum(IC.offset(j)) == 1]


def selected(values, level, invert=False):
    return IC.is_inside(values, level) != bool(invert)


def label_mask(sel, connectivity=14):
    """Components of the True points of sel (N0,N1,N2) -> labels (N0,N1,N2) int32: -1 where False, else the smallest flat index of the
    component."""
    sel = np.asarray(sel, bool)
    n = sel.size
    lab = np.where(sel, np.arange(n).reshape(sel.shape), n).astype(np.int64)
    pairs = []
    for d in kinds(connectivity):
        own = tuple(slice(0, s - dd) for s, dd in zip(sel.shape, d))
        oth = tuple(slice(dd, s) for s, dd in zip(sel.shape, d))
        pairs.append((own, oth, sel[own] & sel[oth]))
    flat_sel = np.nonzero(sel.ravel())[0]
    while True:
        new = lab.copy()
        for own, oth, both in pairs:
            m = np.minimum(new[own], new[oth])
            new[own] = np.where(both, m, new[own])
            new[oth] = np.where(both, np.minimum(m, new[oth]), new[oth])      # (own and oth overlap: own's update may be below m already)
        # pointer jumping: a label is the index of a point of the same component, whose own label is no larger
        flat = new.ravel()
        while True:
            hop = flat[flat[flat_sel]]
            if np.array_equal(hop, flat[flat_sel]):
                break
            flat[flat_sel] = hop
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(sel, lab, -1).astype(np.int32)


def sizes_and_stats(labels):
    """sizes (N0,N1,N2) int32: the point count at each root; stats int32[4]: components, largest root (lowest at equal size, -1 if none),
    its size, status 0."""
    lab = labels.ravel()
    sizes = np.bincount(lab[lab >= 0], minlength=lab.size).astype(np.int32)
    k = int((sizes > 0).sum())
    root = int(np.argmax(sizes)) if k else -1                       # argmax: the first, that is the lowest, of the largest
    stats = np.array([k, root, int(sizes[root]) if k else 0, 0], np.int32)
    return sizes.reshape(labels.shape), stats


def label(values, level, invert=False, connectivity=14):
    labels = label_mask(selected(values, level, invert), connectivity)
    return (labels,) + sizes_and_stats(labels)


def filter_values(values, labels, sizes, stats, largest_only, min_size, fill):
    """cnerf_components_filter: values, but fill where a labelled point's component is smaller than min_size or (largest_only) is not
    the largest."""
    out = np.array(values, F, copy=True)
    lab = labels.ravel()
    on = lab >= 0
    root = np.where(on, lab, 0)
    bad = on & ((sizes.ravel()[root] < min_size) | (bool(largest_only) & (root != stats[1])))
    out.ravel()[bad] = F(fill)
    return out


def keep(values, level, largest=True, min_size=0, fill=None, invert=False, connectivity=14):
    if fill is None:
        fill = np.inf if invert else -np.inf
    return filter_values(values, *label(values, level, invert, connectivity), largest, min_size, fill)


def same_partition(a, b):
    """Two labelings (any ids; a negative or zero id of b / a negative id of a = not labelled) cut the lattice into the same pieces."""
    a, b = np.asarray(a).ravel(), np.asarray(b).ravel()
    if not np.array_equal(a >= 0, b > 0):
        return False
    on = a >= 0
    pa, pb = a[on], b[on]
    pairs = np.unique(np.stack([pa, pb], 1), axis=0)
    return len(pairs) == len(np.unique(pa)) == len(np.unique(pb))


def triangle_keys(vertices, faces):
    """Every triangle as the bits of its three vertices, in the order the face lists them."""
    v = np.ascontiguousarray(vertices, F).view(np.uint32)
    return {tuple(row) for row in v[np.asarray(faces, np.int64)].reshape(len(faces), 9).tolist()}


def is_submesh(mesh, of):
    """Every triangle of `mesh`, as vertex bit triples, is a triangle of `of`."""
    return triangle_keys(mesh[0], mesh[1]) <= triangle_keys(of[0], of[1])


# ---------------------------------------------------------------------------------------------------------------------
# lattices
# ---------------------------------------------------------------------------------------------------------------------
def ball_and_floaters(N, n_floaters, seed, radius=0.3, small=0.04):
    """A ball about the centre of the unit cube (pitch 1 / (N - 1)) and n_floaters small balls in the shell outside it: positive inside."""
    rng = np.random.default_rng(seed)
    pitch = 1.0 / (N - 1)
    x = IC.positions((N, N, N), (0.0, 0.0, 0.0), pitch).astype(np.float64)
    v = radius ** 2 - ((x - 0.5) ** 2).sum(-1)
    for _ in range(n_floaters):
        c = rng.uniform(0.05, 0.95, 3)
        if np.linalg.norm(c - 0.5) < radius + 2.5 * small:
            continue
        v = np.maximum(v, small ** 2 - ((x - c) ** 2).sum(-1))
    return v.astype(F), pitch


def hollow_ball(N=24, r_in=0.2, r_out=0.4):
    """1 where r_in < r < r_out about the centre of the unit cube, else -1 (pitch 1 / (N - 1)); smoothed by the distance to the shell's
    mid surface so that the level set is round: value = half thickness - |r - mid radius|."""
    pitch = 1.0 / (N - 1)
    x = IC.positions((N, N, N), (0.0, 0.0, 0.0), pitch).astype(np.float64)
    r = np.linalg.norm(x - 0.5, axis=-1)
    return (0.5 * (r_out - r_in) - np.abs(r - 0.5 * (r_out + r_in))).astype(F), pitch


def winding_path(A=16, B=16, M=16):
    """One path that winds through a (2A-1, 2B-1, M) lattice: the rows along axis 2 at even (i0, i1), joined end to end in boustrophedon
    order by single points (at odd i1 inside a plane, at odd i0 between planes).  Rows are two apart, so nothing else touches under
    either neighbourhood but for the corner diagonal at each joint.  1 on the path, 0 off it; A B M + A B - 1 points, root 0."""
    v = np.zeros((2 * A - 1, 2 * B - 1, M), F)
    end = 0                                                        # the i2 end at which the next joint sits: a row is run 0 -> M-1 or back
    for a in range(A):
        bs = range(B) if a % 2 == 0 else range(B - 1, -1, -1)
        for k, b in enumerate(bs):
            v[2 * a, 2 * b, :] = 1
            end = M - 1 - end
            if k + 1 < B:
                v[2 * a, 2 * b + (1 if a % 2 == 0 else -1), end] = 1
            elif a + 1 < A:
                v[2 * a + 1, 2 * b, end] = 1
    return v


def smoothed_noise(N, seed, passes=2):
    """White noise averaged over the 3x3x3 box `passes` times (periodic), scaled to unit deviation."""
    v = np.random.default_rng(seed).standard_normal((N, N, N))
    for _ in range(passes):
        for ax in range(3):
            v = (np.roll(v, 1, ax) + v + np.roll(v, -1, ax)) / 3.0
    return (v / v.std()).astype(F)
