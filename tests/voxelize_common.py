"""NumPy statements of cnerf_voxelize and cnerf_voxel_first_hit (include/cnerf.h), float32 operation by operation -- voxelize32,
first_hit32 -- and float64 statements of what the reference computes: open3d's VoxelGrid as feature_volume/pcl2voxel.py uses it
(open3d_f64) and the march of feature_volume/voxel2img.py (interpolate_f64).  Written from the contracts."""
import numpy as np

from render_rays_common import linspace32

F = np.float32
Q = F(16777216.0)       # 2^24


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def clamp_lengths(lengths, B, n):
    return np.full(B, n, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, n)


def quantise(c):
    """q of the contract, uint64."""
    c = np.where(np.isnan(c), F(0), c.astype(F))
    return np.rint((np.fmin(np.fmax(c, F(0)), F(1)) * Q).astype(F)).astype(np.uint64)


def cells32(xyz, G, lo, side, clip_margin):
    """-> (keep (n,) bool, ijk (n,3) int64) of float32 positions (n,3)."""
    xyz = xyz.astype(F)
    lo = np.broadcast_to(np.asarray(lo, F), (3,))
    side = F(side)
    inv = F(F(G) / side)
    keep = ~np.isnan(xyz).any(1)
    with np.errstate(invalid="ignore", over="ignore"):
        if clip_margin is not None and clip_margin >= 0:
            m = F(clip_margin)
            c_lo = (lo + m).astype(F)
            c_hi = ((lo + side).astype(F) - m).astype(F)
            p = np.fmin(np.fmax(xyz, c_lo), c_hi)
            t = ((p - lo).astype(F) * inv).astype(F)
            ijk = np.clip(np.floor(np.where(keep[:, None], t, F(0))), 0, G - 1).astype(np.int64)
        else:
            t = ((xyz - lo).astype(F) * inv).astype(F)
            keep &= ((t >= 0) & (t < F(G))).all(1)
            ijk = np.floor(np.where(keep[:, None], t, F(0))).astype(np.int64)
    return keep, ijk


def voxelize32(points, G, lo, side, lengths=None, clip_margin=1e-4, layout=0):
    """points (B,n,stride >= 6) -> voxels float32 in `layout` (0: (B,4,G,G,G) [b,ch,iz,iy,ix]; 1: (B,G,G,G,4) [b,ix,iy,iz,ch]) and
    counts int32 (B,G,G,G) in the layout's spatial order."""
    points = np.asarray(points, F)
    B, n = points.shape[:2]
    np_ = clamp_lengths(lengths, B, n)
    vox = np.zeros((B, G, G, G, 4), F)          # [b, ix, iy, iz, ch]
    cnt = np.zeros((B, G, G, G), np.int32)
    for b in range(B):
        rows = points[b, :np_[b]]
        keep, ijk = cells32(rows[:, :3], G, lo, side, clip_margin)
        flat = ((ijk[:, 0] * G + ijk[:, 1]) * G + ijk[:, 2])[keep]
        c = np.bincount(flat, minlength=G ** 3)
        cnt[b] = c.reshape(G, G, G)
        occ = c > 0
        vox[b, ..., 0] = occ.reshape(G, G, G)
        for ch in range(3):
            q = quantise(rows[keep, 3 + ch])
            s = np.bincount(flat, weights=q.astype(np.float64), minlength=G ** 3)       # integers below 2^53: exact in any order
            assert s.max(initial=0) < 2.0 ** 52
            col = np.zeros(G ** 3, F)
            col[occ] = (s[occ] / (c[occ].astype(np.float64) * 16777216.0)).astype(F)
            vox[b, ..., 1 + ch] = col.reshape(G, G, G)
    if layout == 0:
        return np.ascontiguousarray(vox.transpose(0, 4, 3, 2, 1)), np.ascontiguousarray(cnt.transpose(0, 3, 2, 1))
    return vox, cnt


def grid_xyzc(voxels, layout):
    """Either layout -> [b, ix, iy, iz, ch]."""
    v = np.asarray(voxels, F)
    return v.transpose(0, 4, 3, 2, 1) if layout == 0 else v


def first_hit32(voxels, origins, dirs, lo, side, t_min, t_max, S, background=(1, 1, 1), layout=0):
    """-> pixels (B,P,3) float32, hit_t (B,P) float32, hit_cell (B,P) int32."""
    v = grid_xyzc(voxels, layout)
    B, G = v.shape[0], v.shape[1]
    o, d = np.asarray(origins, F), np.asarray(dirs, F)
    lo = np.broadcast_to(np.asarray(lo, F), (3,))
    inv = F(F(G) / F(side))
    ts = linspace32(t_min, t_max, S)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (o[:, :, None, :] + (d[:, :, None, :] * ts[None, None, :, None]).astype(F)).astype(F)       # (B,P,S,3)
        t = ((p - lo).astype(F) * inv).astype(F)
        inside = ((t >= 0) & (t < F(G))).all(-1)
        ijk = np.floor(np.where(inside[..., None], t, F(0))).astype(np.int64)
    bi = np.arange(B)[:, None, None]
    cell = v[bi, ijk[..., 0], ijk[..., 1], ijk[..., 2]]                 # (B,P,S,4)
    occupied = inside & (cell[..., 0] != 0)                             # a NaN is occupied
    hit = occupied.any(-1)
    first = occupied.argmax(-1)
    pick = np.take_along_axis(cell, first[..., None, None], 2)[:, :, 0]
    flat = (ijk[..., 0] * G + ijk[..., 1]) * G + ijk[..., 2]
    pixels = np.where(hit[..., None], pick[..., 1:], np.asarray(background, F)).astype(F)
    hit_t = np.where(hit, ts[first], F(np.inf)).astype(F)
    hit_cell = np.where(hit, np.take_along_axis(flat, first[..., None], 2)[..., 0], -1).astype(np.int32)
    return pixels, hit_t, hit_cell


# ---------------------------------------------------------------------------------------------------------------------
# what the reference computes, in float64
# ---------------------------------------------------------------------------------------------------------------------
def open3d_t64(xyz, G, length):
    """The real cell coordinate of pcl2voxel.py's clipped positions: (clip(p) - min_bound) / voxel_size, voxel_size = length / G."""
    p = np.clip(np.asarray(xyz, np.float64), -length / 2 + 1e-4, length / 2 - 1e-4)
    return (p - (-length / 2)) / (length / G)


def open3d_f64(points, G, length):
    """points (n,6) -> counts (G,G,G) int64 and mean colours (G,G,G,3) float64 indexed [ix,iy,iz]: a point's voxel is
    floor((p - min_bound) / voxel_size), a voxel's colour the mean of its points' colours clipped to [0,1] (pcl2voxel.py:40-41,53-64)."""
    points = np.asarray(points, np.float64)
    ijk = np.floor(open3d_t64(points[:, :3], G, length)).astype(np.int64)
    assert ijk.min() >= 0 and ijk.max() < G
    flat = (ijk[:, 0] * G + ijk[:, 1]) * G + ijk[:, 2]
    c = np.bincount(flat, minlength=G ** 3)
    col = np.zeros((G ** 3, 3))
    rgb = np.clip(points[:, 3:6], 0, 1)
    for ch in range(3):
        s = np.bincount(flat, weights=rgb[:, ch], minlength=G ** 3)
        col[c > 0, ch] = s[c > 0] / c[c > 0]
    return c.reshape(G, G, G), col.reshape(G, G, G, 3)


def interpolate_u64(origins, dirs, length, G, t_min, t_max, S):
    """The unrounded voxel coordinate of voxel2img's samples, (B,P,S,3) float64: grid_sample(align_corners=False) places the normalised
    x = p / (length / 2) at ((x + 1) G - 1) / 2, and mode='nearest' rounds that to the nearest integer."""
    ts = np.linspace(np.float64(F(t_min)), np.float64(F(t_max)), S)
    p = np.asarray(origins, np.float64)[:, :, None, :] + np.asarray(dirs, np.float64)[:, :, None, :] * ts[None, None, :, None]
    return ((p / (length / 2) + 1) * G - 1) / 2


def interpolate_f64(voxels, origins, dirs, length, t_min, t_max, S, layout=0):
    """voxel2img.voxel_interpolate: per ray the colour of the first sample whose nearest voxel has sigma != 0, else white.  The nearest
    index is clamped into the grid (padding_mode='border')."""
    v = grid_xyzc(voxels, layout)
    B, G = v.shape[0], v.shape[1]
    ijk = np.clip(np.rint(interpolate_u64(origins, dirs, length, G, t_min, t_max, S)), 0, G - 1).astype(np.int64)
    cell = v[np.arange(B)[:, None, None], ijk[..., 0], ijk[..., 1], ijk[..., 2]]
    occupied = cell[..., 0] != 0
    hit = occupied.any(-1)
    pick = np.take_along_axis(cell, occupied.argmax(-1)[..., None, None], 2)[:, :, 0]
    return np.where(hit[..., None], pick[..., 1:], F(1)).astype(F)
