"""NumPy statements of the contract of csrc/tsdf.hip as include/cnerf.h words it: tsdf32 in float32, operation by operation in the header's
order, every operation rounded on its own; tsdf64, the same decisions in float64 on the float32 inputs; and the analytic depth maps of a
ball.  Test infrastructure only."""
import numpy as np

import isosurface_common as IC
import reproject_common as RC

F = np.float32
U = RC.U24


def tsdf32(shape, lo, pitch, depth, cams, focal, z_min, z_max, trunc, colors=None, color_layout=0, color_scale=1.0, color_offset=0.0, carve=True,
           hidden_min=1, unseen=-1.0):
    """-> tsdf (n0,n1,n2) float32, weight (n0,n1,n2) int32, rgb (n0,n1,n2,3) float32 or None."""
    depth = np.asarray(depth, F)
    V, R, _ = depth.shape
    M = np.asarray(cams, F).reshape(V, 4, 4)
    pos = IC.positions(shape, lo, pitch).reshape(-1, 3)
    nvox = len(pos)
    total = np.zeros(nvox, F)
    n, hidden, cn = np.zeros(nvox, np.int32), np.zeros(nvox, np.int32), np.zeros(nvox, np.int32)
    csum = np.zeros((nvox, 3), F)
    if colors is not None:
        colors = np.asarray(colors, F)
    for w in range(V):
        z, u, v = RC.project32(pos, M[w], focal, R)
        with np.errstate(invalid="ignore"):
            ok = z > F(0)
            ok &= (F(-1) < u) & (u < F(R)) & (F(-1) < v) & (v < F(R))
        col, row = np.rint(np.where(ok, u, 0)).astype(np.int64), np.rint(np.where(ok, v, 0)).astype(np.int64)
        ok &= (col >= 0) & (col < R) & (row >= 0) & (row < R)
        col, row = np.where(ok, col, 0), np.where(ok, row, 0)
        d = depth[w, row, col]
        with np.errstate(all="ignore"):
            surface = ok & (F(z_min) < d) & (d < F(z_max))
            s = ((z - d).astype(F) / F(trunc)).astype(F)
            hid = surface & (s > F(1))
            obs = surface & ~hid
            if colors is not None:
                band = obs & (s >= F(-1))
                c = colors[w][:, row, col].T if color_layout == 0 else colors[w][row, col, :]
                c = (c * F(color_scale)).astype(F) + F(color_offset)
                csum = np.where(band[:, None], (csum + c).astype(F), csum)
                cn += band
            total = np.where(obs, (total + np.fmax(s, F(-1))).astype(F), total)
            background = ok & ~surface & ~np.isnan(d) & bool(carve)
            total = np.where(background, (total + F(-1)).astype(F), total)
        hidden += hid
        n += obs | background
    with np.errstate(all="ignore"):
        solid = (hidden >= hidden_min) if hidden_min > 0 else np.zeros(nvox, bool)
        tsdf = np.where(n > 0, total / n.astype(F), np.where(solid, F(1), F(unseen))).astype(F)
        weight = np.where(n > 0, n, -hidden).astype(np.int32)
        rgb = None
        if colors is not None:
            rgb = np.where((cn > 0)[:, None], csum / cn.astype(F)[:, None], F(0)).astype(F).reshape(*shape, 3)
    return tsdf.reshape(shape), weight.reshape(shape), rgb


def positions64(shape, lo, pitch):
    """(n,3) float64: i_c * pitch + lo_c of the float32 pitch and lo, without the two roundings of the float32 position."""
    axes = [np.arange(n) * np.float64(F(pitch)) + np.float64(F(l)) for n, l in zip(shape, lo)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)


def tsdf64(shape, lo, pitch, depth, cams, focal, z_min, z_max, trunc, carve=True, hidden_min=1, unseen=-1.0):
    """The same decisions in float64 on the float32 inputs (lo, pitch, depth, cameras, focal, trunc).
    -> tsdf (n0,n1,n2) float64, weight int32, and per view a dict of the float64 z, u, v, the depth read d, `ok` (the view reads a
    pixel), `surface`, `obs` (the view observes a clamped s) for every voxel."""
    depth = np.asarray(depth, F)
    V, R, _ = depth.shape
    M = np.asarray(cams, F).reshape(V, 4, 4)
    pos = positions64(shape, lo, pitch)
    nvox = len(pos)
    total = np.zeros(nvox)
    n, hidden = np.zeros(nvox, np.int32), np.zeros(nvox, np.int32)
    views = []
    t64 = np.float64(F(trunc))
    for w in range(V):
        z, u, v = RC.project64(pos, M[w], F(focal), R)
        with np.errstate(invalid="ignore"):
            ok = (z > 0) & (-1 < u) & (u < R) & (-1 < v) & (v < R)
        col, row = np.rint(np.where(ok, u, 0)).astype(np.int64), np.rint(np.where(ok, v, 0)).astype(np.int64)
        ok &= (col >= 0) & (col < R) & (row >= 0) & (row < R)
        col, row = np.where(ok, col, 0), np.where(ok, row, 0)
        d = depth[w, row, col].astype(np.float64)
        with np.errstate(all="ignore"):
            surface = ok & (np.float64(F(z_min)) < d) & (d < np.float64(F(z_max)))
            s = (z - d) / t64
            hid = surface & (s > 1)
            obs = surface & ~hid
            total = np.where(obs, total + np.fmax(s, -1.0), total)
            background = ok & ~surface & ~np.isnan(d) & bool(carve)
            total = np.where(background, total - 1.0, total)
        hidden += hid
        n += obs | background
        views.append(dict(z=z, u=u, v=v, d=d, ok=ok, surface=surface, obs=obs))
    with np.errstate(all="ignore"):
        solid = (hidden >= hidden_min) if hidden_min > 0 else np.zeros(nvox, bool)
        tsdf = np.where(n > 0, total / n, np.where(solid, 1.0, np.float64(F(unseen))))
    return tsdf.reshape(shape), np.where(n > 0, n, -hidden).astype(np.int32).reshape(shape), views


def sphere_depth(cams, R, focal, r):
    """(V,R,R) float32: the z-depth at which the ray of pixel (row, col) of each camera first meets the ball of radius r about the origin,
    evaluated in float64 and rounded; 0 where the ray misses.  The ray is the back-projection's: camera-space direction
    (xn / focal, yn / focal, 1), xn = (2 col - (R-1)) / (R-1), so its parameter IS the z-depth."""
    cams = np.asarray(cams, F).reshape(-1, 4, 4).astype(np.float64)
    g = (2 * np.arange(R) - (R - 1)) / (R - 1) / np.float64(focal)
    dirs = np.stack([np.broadcast_to(g[None, :], (R, R)), np.broadcast_to(g[:, None], (R, R)), np.ones((R, R))], -1)      # [row, col] -> (x, y, 1)
    out = np.zeros((len(cams), R, R), F)
    for w, Mw in enumerate(cams):
        dw = dirs @ Mw[:3, :3].T
        o = Mw[:3, 3]
        a, b, c = (dw * dw).sum(-1), (dw * o).sum(-1), (o * o).sum() - r * r
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            lam = (-b - np.sqrt(disc)) / a
        out[w] = np.where((disc > 0) & (lam > 0), lam, 0.0).astype(F)
    return out


def sphere_pixels(cams, R, focal, r):
    """(V,3,R,R) float32 in [-1,1]: the unit normal of the ball where sphere_depth hits it, 0 elsewhere -- a colour that varies over the
    surface and that 0.5 c + 0.5 brings into [0,1]."""
    cams4 = np.asarray(cams, F).reshape(-1, 4, 4).astype(np.float64)
    d = sphere_depth(cams, R, focal, r).astype(np.float64)
    g = (2 * np.arange(R) - (R - 1)) / (R - 1) / np.float64(focal)
    dirs = np.stack([np.broadcast_to(g[None, :], (R, R)), np.broadcast_to(g[:, None], (R, R)), np.ones((R, R))], -1)
    out = np.zeros((len(cams4), 3, R, R), F)
    for w, Mw in enumerate(cams4):
        p = (dirs * d[w][..., None]) @ Mw[:3, :3].T + Mw[:3, 3]
        out[w] = np.where(d[w] > 0, p.transpose(2, 0, 1) / r, 0.0).astype(F)
    return out


def components(n_vertices, faces):
    """Number of connected components of a mesh's vertices that a face touches (labels flow along the edges until nothing changes)."""
    f = np.asarray(faces, np.int64)
    label = np.arange(n_vertices)
    while True:
        low = label[f].min(1)
        new = label.copy()
        for k in range(3):
            np.minimum.at(new, f[:, k], low)
        new = new[new]                                  # a hop of pointer jumping
        if np.array_equal(new, label):
            break
        label = new
    return len(np.unique(label[np.unique(f)]))
