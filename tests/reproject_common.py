"""NumPy statements of the two contracts of csrc/reproject.hip as include/cnerf.h words them -- backproject32 and splat32, float32,
operation by operation in the header's order, every operation rounded on its own -- and float64 statements of what the reference
computes: the lift of Inferencer.render_pcl (inference.py:543-558) and its inverse, the pinhole projection.  Test infrastructure only."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
U24 = 2.0 ** -24            # the unit roundoff of float32


def focal32(fov=49.134342641202636):
    """1 / tan(fov / 2) as volumetric_rendering.pinhole_rays forms it: the double tangent rounded to fp32, then 1 / x in fp32."""
    return F(1.0) / F(np.tan((2 * np.pi * fov / 360) / 2))


def look_at(origins):
    """create_cam2world_matrix(origin, "y") in float64 NumPy, returned as float32 (V,4,4): rotation columns (-left, -up, forward),
    translation = origin.  A rotation to float32 rounding."""
    o = np.asarray(origins, np.float64)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    fwd = unit(-o)
    left = unit(np.cross(np.broadcast_to([0.0, 1.0, 0.0], fwd.shape), fwd))
    up = unit(np.cross(fwd, left))
    M = np.tile(np.eye(4), (len(o), 1, 1))
    M[:, :3, 0], M[:, :3, 1], M[:, :3, 2], M[:, :3, 3] = -left, -up, fwd, o
    return M.astype(F)


def cameras(n, seed, r_lo=0.9, r_hi=1.3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 1] = np.clip(d[:, 1], -0.9, 0.9)                      # away from the poles of the look-at
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return look_at(d * rng.uniform(r_lo, r_hi, (n, 1)))


# ---------------------------------------------------------------------------------------------------------------------
# back-projection
# ---------------------------------------------------------------------------------------------------------------------
def valid32(depth, z_min, z_max, mask=None, mask_min=0.0):
    z = np.asarray(depth, F)
    with np.errstate(invalid="ignore"):
        ok = (F(z_min) < z) & (z < F(z_max))
        if mask is not None:
            ok &= np.asarray(mask, F) > F(mask_min)
    return ok


def backproject32(depth, cams, focal, z_min, z_max, colors=None, color_layout=0, color_scale=1.0, color_offset=0.0, mask=None, mask_min=0.0):
    """-> points (n, 6 or 3) float32, counts (V) int32, pixel (n) int32, rank (V,R,R) int32."""
    depth = np.asarray(depth, F)
    V, R, _ = depth.shape
    M = np.asarray(cams, F).reshape(V, 4, 4)
    ok = valid32(depth, z_min, z_max, mask, mask_min)
    v, row, col = np.nonzero(ok)                               # ascending (v, row, col)
    z = depth[v, row, col]
    Rm1, f = F(R - 1), F(focal)
    xn = (2 * col - (R - 1)).astype(F) / Rm1
    yn = (2 * row - (R - 1)).astype(F) / Rm1
    xc = (xn / f) * z
    yc = (yn / f) * z
    cols = [((M[v, i, 0] * xc + M[v, i, 1] * yc) + M[v, i, 2] * z) + M[v, i, 3] for i in range(3)]
    if colors is not None:
        c = np.asarray(colors, F)
        c = c[v, :, row, col] if color_layout == 0 else c[v, row, col, :]
        cols += [c[:, k] * F(color_scale) + F(color_offset) for k in range(3)]
    points = np.stack(cols, 1).astype(F) if len(v) else np.zeros((0, len(cols)), F)
    counts = ok.reshape(V, -1).sum(1).astype(np.int32)
    pixel = ((v * R + row) * R + col).astype(np.int32)
    rank = np.full((V, R, R), -1, np.int32)
    rank[v, row, col] = np.arange(len(v), dtype=np.int32)
    return points, counts, pixel, rank


def backproject64(depth, cams, focal, z_min, z_max):
    """inference.py:543-558 in float64 on the float32 inputs: yx = (2 nonzero - (R-1)) / (R-1) / focal * depth, pts = [x, y, depth, 1],
    world = pts @ cam.T.  -> world (n,3), and the magnitudes of the four addends of every coordinate (n,3,4): the scale of the bound."""
    depth = np.asarray(depth, F)
    V, R, _ = depth.shape
    M = np.asarray(cams, F).reshape(V, 4, 4).astype(np.float64)
    v, row, col = np.nonzero(valid32(depth, z_min, z_max))
    z = depth[v, row, col].astype(np.float64)
    xc = (2 * col - (R - 1)) / (R - 1) / np.float64(focal) * z
    yc = (2 * row - (R - 1)) / (R - 1) / np.float64(focal) * z
    pts = np.stack([xc, yc, z, np.ones_like(z)], 1)
    world = np.einsum("nij,nj->ni", M[v], pts)[:, :3]
    return world, np.abs(M[v][:, :3, :]) * np.abs(pts)[:, None, :]


def lift64(M, row, col, z, R, focal):
    """World position (float32) of the point at camera depth z whose projection is pixel (row, col) -- fractions allowed -- of camera M."""
    M = np.asarray(M, np.float64)
    cam = np.asarray([(2 * col - (R - 1)) / (R - 1) / float(focal) * z, (2 * row - (R - 1)) / (R - 1) / float(focal) * z, z, 1.0])
    return (M @ cam)[:3].astype(F)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------
# z-buffered splat
# ---------------------------------------------------------------------------------------------------------------------
def project32(p, M, focal, R):
    """One view, float32 in the header's order: points (n,3), M (4,4) -> z, u, v (n)."""
    p, M = np.asarray(p, F), np.asarray(M, F)
    f = F(focal)
    with np.errstate(all="ignore"):
        q = [p[:, k] - M[k, 3] for k in range(3)]
        cam = [(q[0] * M[0, j] + q[1] * M[1, j]) + q[2] * M[2, j] for j in range(3)]
        z = cam[2]
        half = F(0.5) * F(R - 1)
        u = ((cam[0] * f) / z) * half + half
        v = ((cam[1] * f) / z) * half + half
    return z, u, v


def project64(p, M, focal, R):
    """The inverse of the lift in float64: cam = R^T (p - t), u = cam_x focal / z * (R-1)/2 + (R-1)/2."""
    p, M = np.asarray(p, np.float64), np.asarray(M, np.float64)
    cam = (p[:, :3] - M[:3, 3]) @ M[:3, :3]
    z = cam[:, 2]
    half = 0.5 * (R - 1)
    with np.errstate(all="ignore"):
        return z, cam[:, 0] * np.float64(focal) / z * half + half, cam[:, 1] * np.float64(focal) / z * half + half


def footprint(keys, R, row, col, key, radius):
    """keys (R*R) uint64: minimum with `key` over the pixels (row + dr, col + dc), |dr|, |dc| <= radius, inside the image."""
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            rr, cc = row + dr, col + dc
            ok = (rr >= 0) & (rr < R) & (cc >= 0) & (cc < R)
            np.minimum.at(keys, rr[ok] * R + cc[ok], key[ok])


def splat32(points, cams, R, focal, z_min, z_max, radius=0, lengths=None, background=(1.0, 1.0, 1.0)):
    """points (B,n,stride), cams (B,V,4,4) -> depth (B,V,R,R) float32, index int32, pixels (B,V,R,R,3) (None when stride < 6)."""
    points = np.asarray(points, F)
    B, n, stride = points.shape
    cams = np.asarray(cams, F).reshape(B, -1, 4, 4)
    V = cams.shape[1]
    depth = np.zeros((B, V, R, R), F)
    index = np.full((B, V, R, R), -1, np.int32)
    pixels = np.empty((B, V, R, R, 3), F) if stride >= 6 else None
    if pixels is not None:
        pixels[:] = np.asarray(background, F)
    for b in range(B):
        np_ = n if lengths is None else min(max(int(lengths[b]), 0), n)
        for w in range(V):
            z, u, v = project32(points[b, :np_, :3], cams[b, w], focal, R)
            with np.errstate(invalid="ignore"):
                keep = (F(z_min) < z) & (z < F(z_max))
                lo, hi = F(-(radius + 1)), F(R + radius)
                keep &= (lo < u) & (u < hi) & (lo < v) & (v < hi)
            i = np.nonzero(keep)[0]
            col, row = np.rint(u[i]).astype(np.int64), np.rint(v[i]).astype(np.int64)
            key = (z[i].view(np.uint32).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)
            keys = np.full(R * R, EMPTY, np.uint64)
            footprint(keys, R, row, col, key, radius)
            hit = keys != EMPTY
            win = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            depth[b, w].reshape(-1)[hit] = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(F)
            index[b, w].reshape(-1)[hit] = win
            if pixels is not None:
                pixels[b, w].reshape(-1, 3)[hit] = points[b, win, 3:6]
    return depth, index, pixels


def splat64(points, cams, R, focal, z_min, z_max, radius=0):
    """The same picture in float64, one view per image list: nearest point per pixel (lowest index at equal depth).
    -> depth (B,V,R,R) float64 (0 = nothing), index int32, and per (b, view) the float64 (z, u, v) of every point."""
    points = np.asarray(points, F)
    B, n, _ = points.shape
    cams = np.asarray(cams, F).reshape(B, -1, 4, 4)
    V = cams.shape[1]
    depth = np.zeros((B, V, R, R))
    index = np.full((B, V, R, R), -1, np.int32)
    proj = {}
    for b in range(B):
        for w in range(V):
            z, u, v = project64(points[b], cams[b, w], focal, R)
            proj[b, w] = (z, u, v)
            with np.errstate(invalid="ignore"):
                keep = (z_min < z) & (z < z_max) & (-(radius + 1) < u) & (u < R + radius) & (-(radius + 1) < v) & (v < R + radius)
            i = np.nonzero(keep)[0]
            order = i[np.lexsort((i, z[i]))][::-1]             # farthest first: the last write per pixel is the nearest, lowest index
            col, row = np.rint(u[order]).astype(np.int64), np.rint(v[order]).astype(np.int64)
            d, ix = depth[b, w], index[b, w]
            for dr in range(-radius, radius + 1):
                for dc in range(-radius, radius + 1):
                    rr, cc = row + dr, col + dc
                    ok = (rr >= 0) & (rr < R) & (cc >= 0) & (cc < R)
                    # among the points of ONE offset the last write wins (farthest first); across offsets compare depths
                    cand_d = np.full((R, R), np.inf)
                    cand_i = np.full((R, R), -1, np.int64)
                    cand_d[rr[ok], cc[ok]] = z[order][ok]
                    cand_i[rr[ok], cc[ok]] = order[ok]
                    cur = np.where(ix >= 0, d, np.inf)
                    better = (cand_d < cur) | ((cand_d == cur) & (cand_i >= 0) & (cand_i < ix))
                    d[better], ix[better] = cand_d[better], cand_i[better]
    return depth, index, proj
