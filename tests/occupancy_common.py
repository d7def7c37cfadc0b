"""Shared by tests/test_occupancy_cpu.py and tests/test_gpu_occupancy.py: the NumPy statement of the occupancy semantics of
include/cnerf.h -- inside / cell / live, the bit build, the stable compaction and the expansion -- and the hand-made
edge points.  TEST INFRASTRUCTURE ONLY.

All cell arithmetic is float32 with every operation rounded on its own: inv = float32(G) / float32(side), t = (p - lo) * inv."""
import numpy as np

FILL = np.array([0.0, 0.0, 0.0, -np.inf], np.float32)


def inv_of(G, side):
    return np.float32(np.float32(G) / np.float32(side))


def cell_coords(points, lo, side, G):
    """points (..., 3) float32 -> t (..., 3) float32 = (p - lo) * inv."""
    p = np.asarray(points, np.float32)
    lo = np.asarray(lo, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((p - lo).astype(np.float32) * inv_of(G, side)).astype(np.float32)


def inside(points, lo, side, G):
    """0 <= t < G on all three axes; a NaN is not inside."""
    t = cell_coords(points, lo, side, G)
    with np.errstate(invalid="ignore"):
        return ((t >= np.float32(0)) & (t < np.float32(G))).all(-1)


def cell_index(points, lo, side, G):
    """Bit index (ix G + iy) G + iz of the points that are inside, -1 elsewhere."""
    t = cell_coords(points, lo, side, G)
    ins = inside(points, lo, side, G)
    with np.errstate(invalid="ignore"):
        i = np.where(ins[..., None], np.floor(t), 0).astype(np.int64)
    return np.where(ins, (i[..., 0] * G + i[..., 1]) * G + i[..., 2], -1)


def bit_at(words, idx):
    """Bit idx of a word array (uint32): word idx >> 5, bit idx & 31."""
    words = np.asarray(words).view(np.uint32)
    return ((words[idx >> 5] >> (idx & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def live(points, words, lo, side, G):
    """points (n, 3), words (G^3 / 32) of ONE image -> (n) bool: not inside, or the cell's bit is set."""
    idx = cell_index(points, lo, side, G)
    return (idx < 0) | bit_at(words, np.maximum(idx, 0))


def pack_bits(cells):
    """(..., G^3) bool in bit order -> (..., G^3 / 32) uint32."""
    c = np.asarray(cells, bool).reshape(*np.shape(cells)[:-1], -1, 32)
    return (c.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def build_cells(sigma, G, threshold, dilate):
    """sigma (B, (G+1)^3) at the cell corners -> (B, G^3) bool: m = max over a cell's 8 corners, m' = max of m over the cells within
    `dilate` on every axis (clipped at the grid), set iff not (m' <= threshold).  np.maximum keeps a NaN, so a NaN sets its bits."""
    s = np.asarray(sigma, np.float32).reshape(-1, G + 1, G + 1, G + 1)
    m = s[:, :-1, :-1, :-1]
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                m = np.maximum(m, s[:, dx:dx + G, dy:dy + G, dz:dz + G])
    out = np.empty_like(m)
    for ix in range(G):
        xs = slice(max(ix - dilate, 0), min(ix + dilate, G - 1) + 1)
        for iy in range(G):
            ys = slice(max(iy - dilate, 0), min(iy + dilate, G - 1) + 1)
            for iz in range(G):
                zs = slice(max(iz - dilate, 0), min(iz + dilate, G - 1) + 1)
                out[:, ix, iy, iz] = m[:, xs, ys, zs].reshape(m.shape[0], -1).max(1)       # ndarray.max keeps a NaN too
    with np.errstate(invalid="ignore"):
        return ~(out <= np.float32(threshold)).reshape(out.shape[0], -1)


def build_bits(sigma, G, threshold, dilate):
    return pack_bits(build_cells(sigma, G, threshold, dilate))


def compact(points, words, lo, side, G):
    """points (B, n, 3), words (B, G^3 / 32) -> rank (B, n) int32 (cumsum - 1 over the live points, -1 where skipped), counts (B)."""
    lv = np.stack([live(points[b], words[b], lo, side, G) for b in range(points.shape[0])])
    rank = np.where(lv, np.cumsum(lv, 1) - 1, -1).astype(np.int32)
    return rank, lv.sum(1).astype(np.int32), lv


def expand(rank, live_values):
    """rank (B, n), live_values (B, n, 4) -> (B, n, 4): the live rows at their samples, FILL elsewhere."""
    out = np.broadcast_to(FILL, live_values.shape).copy()
    for b in range(rank.shape[0]):
        k = rank[b] >= 0
        out[b, k] = live_values[b, rank[b, k]]
    return out


def same_bits(a, b):
    """Bit-for-bit equality of two float32 arrays (so that -0.0 != 0.0 and equal NaNs compare equal)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def edge_points(lo, side, G):
    """Hand-made points for the box (lo scalar per axis, side, G): the corner lo itself, lo + side (outside), every cell edge
    lo + k side / G on the x axis, -0.0, NaN, +-inf, a denormal -- the other coordinates at the box centre unless stated."""
    lo32, side32 = np.float32(lo), np.float32(side)
    mid = np.float32(lo32 + side32 * np.float32(0.5))
    rows = [[lo32, lo32, lo32], [np.float32(lo32 + side32)] * 3, [np.float32(lo32 + side32), mid, mid]]
    rows += [[np.float32(lo32 + np.float32(k) * np.float32(side32 / np.float32(G))), mid, mid] for k in range(G + 1)]
    rows += [[np.float32(-0.0), mid, mid], [np.float32(np.nan), mid, mid], [mid, np.float32(np.nan), mid], [np.float32(np.inf), mid, mid],
             [mid, mid, np.float32(-np.inf)], [np.float32(1e-42), mid, mid], [np.float32(-1e-42), np.float32(-0.0), np.float32(0.0)]]
    return np.array(rows, np.float32)


def ball_cells(G, radius_cells):
    """(G^3) bool: cells whose centre lies within radius_cells of the grid's centre."""
    c = np.arange(G, dtype=np.float64) + 0.5 - G / 2
    d2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
    return (d2 <= radius_cells ** 2).reshape(-1)
