"""Shared by tests/test_ray_bounds_cpu.py and tests/test_gpu_ray_bounds.py: the float64 statement of the per-ray bounds contract of
include/cnerf.h (cnerf_occupancy_ray_bounds), the sandwich a fp32 answer has to lie in, the per-ray coarse depths in NumPy
float32, and the ray oracle of tests/render_rays_common.py run on per-ray depths.  TEST INFRASTRUCTURE ONLY.

The reference is brute force: a slab test of every ray against every set cell (fine at G <= 12), in float64 on the float32 inputs."""
import contextlib

import numpy as np
import torch

import occupancy_common as OC
import render_rays_common as RC

ULP = 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------
# the contract in float64
# ---------------------------------------------------------------------------------------------------------------------
def hull_T(origins, dirs, cells, lo, side, G, t_min, t_max, grow=0.0):
    """origins, dirs (n,3); cells (G^3) bool of ONE image in bit order (ix G + iy) G + iz; lo (3).  T = the depths t in [t_min, t_max] at
    which o + t d lies in a set cell, every cell the closed box [lo + i side / G - grow, lo + (i + 1) side / G + grow] per axis.
    t_min, t_max are taken as the float32 numbers the entry receives.
    -> (some (n) bool: T is not empty, inf T (n), sup T (n)); the last two are NaN where T is empty.  A NaN in a ray: T is empty."""
    o, d = np.asarray(origins, np.float64), np.asarray(dirs, np.float64)
    t_min, t_max = np.float64(np.float32(t_min)), np.float64(np.float32(t_max))
    n = o.shape[0]
    idx = np.flatnonzero(np.asarray(cells, bool).reshape(-1))
    some, t_in, t_out = np.zeros(n, bool), np.full(n, np.nan), np.full(n, np.nan)
    if idx.size == 0 or n == 0:
        return some, t_in, t_out
    ijk = np.stack([idx // (G * G), (idx // G) % G, idx % G], -1).astype(np.float64)             # (K,3)
    edge = np.float64(side) / G
    a = np.asarray(lo, np.float64)[None] + ijk * edge - grow                                     # (K,3) lower faces
    b = np.asarray(lo, np.float64)[None] + (ijk + 1) * edge + grow
    lo_t, hi_t = np.full((n, idx.size), np.float64(t_min)), np.full((n, idx.size), np.float64(t_max))
    bad = ~(np.isfinite(o).all(-1) & np.isfinite(d).all(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            ok, dk = o[:, k, None], d[:, k, None]
            ta, tb = (a[None, :, k] - ok) / dk, (b[None, :, k] - ok) / dk
            enter, leave = np.minimum(ta, tb), np.maximum(ta, tb)
            still = dk == 0                                            # never moves on this axis: inside the slab for every t, or for none
            inside = (ok >= a[None, :, k]) & (ok <= b[None, :, k])
            enter = np.where(still, np.where(inside, -np.inf, np.inf), enter)
            leave = np.where(still, np.where(inside, np.inf, -np.inf), leave)
            lo_t, hi_t = np.maximum(lo_t, enter), np.minimum(hi_t, leave)
    crossed = (lo_t <= hi_t) & ~bad[:, None]
    some = crossed.any(1)
    t_in = np.where(some, np.where(crossed, lo_t, np.inf).min(1), np.nan)
    t_out = np.where(some, np.where(crossed, hi_t, -np.inf).max(1), np.nan)
    return some, t_in, t_out


def bounds_of(origins, dirs, cells, lo, side, G, t_min, t_max, pad=0.0, grow=0.0):
    """The contract: (near, far, hit) in float64 / bool.  T empty, or far <= near after the clamp: hit = 0 and [t_min, t_max]."""
    some, t_in, t_out = hull_T(origins, dirs, cells, lo, side, G, t_min, t_max, grow)
    t_min, t_max = np.float64(np.float32(t_min)), np.float64(np.float32(t_max))
    near = np.maximum(t_min, np.where(some, t_in, 0.0) - pad)
    far = np.minimum(t_max, np.where(some, t_out, 0.0) + pad)
    hit = some & (far > near)
    return np.where(hit, near, np.float64(t_min)), np.where(hit, far, np.float64(t_max)), hit


def delta_of(origins, lo, side):
    """The margin of the sandwich: 32 * 2^-23 * M, M the largest coordinate magnitude among the (finite) origins and the cube's corners.
    Four roundings each in a crossing depth (side / G, j * cell, + lo, - o; the division's is relative to a depth and smaller) and in a
    position (d t, + o, - lo, * inv), each at most one ulp 2^-23 M of a number no larger than 2 M / 2: 8 ulps, times four for headroom.
    A distance in SPACE: its room in t on axis k is delta / |d_k|, which is how the rounding error of (plane - o_k) / d_k scales too."""
    o = np.asarray(origins, np.float64)
    lo = np.asarray(lo, np.float64)
    M = max(np.abs(o[np.isfinite(o)]).max(initial=0.0), np.abs(lo).max(), np.abs(lo + np.float64(side)).max())
    return 32.0 * ULP * M


def sandwich(origins, dirs, cells, lo, side, G, t_min, t_max, delta):
    """(inner, outer): hull_T for every set cell shrunk / grown by delta."""
    return (hull_T(origins, dirs, cells, lo, side, G, t_min, t_max, -delta), hull_T(origins, dirs, cells, lo, side, G, t_min, t_max, delta))


def sandwich_violations(near, far, hit, inner, outer, t_min, t_max):
    """Rays of an answer (near, far, hit) with pad = 0 that break  hull(T(shrunk)) in [near, far] in hull(T(grown))  where hit is set,
    hit = 1 where T(shrunk) is not empty, hit = 0 where T(grown) is empty, [t_min, t_max] exactly where hit = 0.  -> list of (ray, why)."""
    near, far, hit = np.asarray(near, np.float64), np.asarray(far, np.float64), np.asarray(hit).astype(bool)
    (in_some, in_a, in_b), (out_some, out_a, out_b) = inner, outer
    bad = []
    for r in range(near.shape[0]):
        if in_some[r] and not hit[r]:
            bad.append((r, "missed a ray that crosses the shrunk cells"))
        elif hit[r] and not out_some[r]:
            bad.append((r, "hit a ray that misses the grown cells"))
        elif hit[r]:
            if not (out_a[r] <= near[r] and far[r] <= out_b[r]):
                bad.append((r, f"[{near[r]!r}, {far[r]!r}] not inside the grown hull [{out_a[r]!r}, {out_b[r]!r}]"))
            elif in_some[r] and not (near[r] <= in_a[r] and in_b[r] <= far[r]):
                bad.append((r, f"[{near[r]!r}, {far[r]!r}] does not hold the shrunk hull [{in_a[r]!r}, {in_b[r]!r}]"))
        elif near[r] != np.float32(t_min) or far[r] != np.float32(t_max):
            bad.append((r, f"a missed ray must keep [t_min, t_max], got [{near[r]!r}, {far[r]!r}]"))
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# rays, cubes and occupancy patterns of the sandwich test
# ---------------------------------------------------------------------------------------------------------------------
T_MIN, T_MAX = RC.RAY_START, RC.RAY_END
CUBES = {2.0: (-1.0, -0.9375, -1.0625), 1.5: (-0.75, -0.8125, -0.6875)}      # side -> an asymmetric lo


def hand_made_rays(lo, side):
    """(origins, dirs) (m,3) float32 for the cube: parallel to an axis (with -0.0 components, one of them in a cell plane), starting
    inside the cube, missing the cube, leaving the cube before T_MIN, a NaN direction."""
    lo = np.asarray(lo, np.float32)
    c = lo + np.float32(side) * np.float32(0.5)
    f = np.float32
    rows = [
        ([lo[0] - f(0.5), c[1] + f(0.07), c[2] - f(0.11)], [1.0, -0.0, 0.0]),                 # along +x
        ([c[0] + f(0.03), lo[1] + f(side) + f(0.4), c[2] + f(0.2)], [-0.0, -0.9, -0.0]),      # along -y
        ([c[0], c[1], lo[2] - f(0.3)], [0.0, 0.0, 1.3]),                                      # along +z, x and y in a cell plane
        ([c[0] + f(0.01), c[1] - f(0.02), c[2] + f(0.03)], [0.3, -0.5, 0.7]),                 # starts inside the cube
        ([c[0] - f(0.3), c[1] + f(0.3), c[2]], [-0.0, 0.0, -1.0]),                            # starts inside, parallel to an axis
        ([lo[0] - f(1.0), lo[1] - f(1.0), c[2]], [-1.0, 0.2, 0.1]),                           # misses: points away
        ([lo[0] - f(0.5), lo[1] + f(side) + f(0.5), c[2]], [1.0, 0.0, 0.0]),                  # misses: parallel, outside the slab
        ([lo[0] + f(side) - f(0.05), c[1], c[2]], [1.0, 0.05, 0.0]),                          # leaves the cube at t = 0.05 < T_MIN
        ([lo[0] - f(0.5), c[1], c[2]], [np.nan, 0.0, 0.0]),                                   # a NaN direction
        ([lo[0] - f(0.5), c[1], c[2]], [1.0, np.nan, 0.0]),
    ]
    return np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.float32)


PATTERNS = ("clear", "set", "ball", "sparse")


def pattern_cells(kind, G, seed=0):
    """(G^3) bool: "clear", "set", "ball" (OC.ball_cells, radius 0.3 G) or "sparse" (a random 10 %: spans that are not convex)."""
    if kind == "clear":
        return np.zeros(G ** 3, bool)
    if kind == "set":
        return np.ones(G ** 3, bool)
    if kind == "ball":
        return OC.ball_cells(G, 0.3 * G)
    return np.random.default_rng(seed).random(G ** 3) < 0.1


def sandwich_rays(lo, side, seed):
    """(B = 2, P = 203 + hand-made, 3) float32: RC.random_rays(unnormalised) aimed at the cube's centre region, then the hand-made rays."""
    o, d = RC.random_rays(2, 203, seed, unnormalised=True)
    ho, hd = hand_made_rays(lo, side)
    o = np.concatenate([o.numpy(), np.broadcast_to(ho, (2, *ho.shape))], 1)
    d = np.concatenate([d.numpy(), np.broadcast_to(hd, (2, *hd.shape))], 1)
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# exact cases: lo = -1, side = 2, G = 8 (cell edge 0.25), every crossing depth representable
# ---------------------------------------------------------------------------------------------------------------------
EXACT_T_MIN, EXACT_T_MAX = 0.0625, 4.0


def exact_cases():
    """-> (origins (m,3), dirs (m,3), cells (2, 512) bool, want: {pad: (near (2,m), far (2,m), hit (2,m))}) worked out by hand.
    Image 0 holds a few cells, image 1 every cell."""
    G = 8
    cells = np.zeros((2, G, G, G), bool)
    cells[1] = True
    cells[0, 2:5, 4, 4] = True                  # x in [-0.5, 0.25], y, z in [0, 0.25]: ray 0
    cells[0, 0, 4, 4] = cells[0, 7, 4, 4] = True         # and the two ends of that row: a span that is not convex
    cells[0, 4, 2, 3] = True                    # x in [0, 0.25], y in [-0.5, -0.25], z in [-0.25, 0]: ray 1
    cells[0, 2, 2, 2] = cells[0, 5, 5, 5] = True         # on the diagonal: ray 2
    rays = [
        ([-2.0, 0.125, 0.125], [1.0, -0.0, 0.0]),        # 0 along +x through cell centres: x = -1 at t = 1, x = 1 at t = 3
        ([0.125, -0.375, 3.0], [0.0, -0.0, -2.0]),       # 1 along -z: z = 1 at t = 1, z = 0 at 1.5, z = -0.25 at 1.625, z = -1 at 2
        ([-1.5, -1.5, -1.5], [1.0, 1.0, 1.0]),           # 2 the diagonal: cell (k,k,k) over t in [0.5 + 0.25 k, 0.75 + 0.25 k]
        ([-2.0, 3.0, 0.125], [1.0, 0.0, -0.0]),          # 3 misses the cube
        ([0.125, 0.125, 0.125], [-0.0, 1.0, 0.0]),       # 4 starts inside set cell (4,4,4): y = 0.1875 at t_min, y = 0.25 at t = 0.125
        ([0.96875, 0.125, 0.125], [1.0, 0.0, 0.0]),      # 5 leaves the cube at t = 0.03125 < t_min
        ([-2.0, 0.125, 0.125], [np.nan, 0.0, 0.0]),      # 6 a NaN
        ([2.0, 0.125, 0.125], [-0.5, 0.0, -0.0]),        # 7 ray 0 backwards at half speed: x = 1 at t = 2, x = -1 at t = 6 > t_max
    ]
    o, d = np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)
    lo_, hi_ = EXACT_T_MIN, EXACT_T_MAX
    want0 = {
        # image 0
        0: [(1.0, 3.0, 1), (1.5, 1.625, 1), (1.0, 2.0, 1), (lo_, hi_, 0), (lo_, 0.125, 1), (lo_, hi_, 0), (lo_, hi_, 0), (2.0, hi_, 1)],
        # image 1: the whole cube
        1: [(1.0, 3.0, 1), (1.0, 2.0, 1), (0.5, 2.5, 1), (lo_, hi_, 0), (lo_, 0.875, 1), (lo_, hi_, 0), (lo_, hi_, 0), (2.0, hi_, 1)],
    }
    pad = 0.125
    want_pad = {b: [(max(lo_, n - pad), min(hi_, f + pad), h) if h else (n, f, h) for n, f, h in rows] for b, rows in want0.items()}
    pack = lambda w: tuple(np.array([[row[i] for row in w[b]] for b in (0, 1)], np.float64) for i in range(3))
    return o, d, cells.reshape(2, -1), {0.0: pack(want0), pad: pack(want_pad)}


# ---------------------------------------------------------------------------------------------------------------------
# per-ray coarse depths in NumPy float32, and the ray oracle on them
# ---------------------------------------------------------------------------------------------------------------------
def linspace32_rays(near, far, S):
    """RC.linspace32 per ray: near, far (...) -> (..., S) float32, torch.linspace(near, far, S) as ATen computes it."""
    near, far = np.asarray(near, np.float32)[..., None], np.asarray(far, np.float32)[..., None]
    step = ((far - near).astype(np.float32) / np.float32(S - 1)).astype(np.float32)
    i = np.arange(S)
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    lo = fma(step, i.astype(np.float32)[None], near)
    hi = fma(-step, (S - 1 - i).astype(np.float32)[None], far)
    return np.where(i < S // 2, lo, hi).astype(np.float32)


def bounded_depths(u, S, near, far):
    """coarse_z (B,P,S) float32 of the bounded sampler: zl[s] + (u - 0.5) (zl[1] - zl[0]), zl = linspace32_rays(near, far, S)."""
    zl = linspace32_rays(near, far, S)
    dz01 = (zl[..., 1] - zl[..., 0]).astype(np.float32)[..., None]
    off = ((np.asarray(u, np.float32) - np.float32(0.5)).astype(np.float32) * dz01).astype(np.float32)
    return (zl + off).astype(np.float32)


def random_bounds(B, P, seed, shortest=0.01):
    """ray_start <= near < far <= ray_end per ray, spans from `shortest` of the interval (every fourth ray) to all of it."""
    g = np.random.default_rng(seed)
    full = np.float64(RC.RAY_END) - np.float64(RC.RAY_START)
    span = g.uniform(0.1, 1.0, (B, P)) * full
    span.reshape(-1)[::4] = g.uniform(shortest, 2 * shortest, span.reshape(-1)[::4].shape) * full
    near = RC.RAY_START + g.random((B, P)) * (full - span)
    near, far = near.astype(np.float32), (near + span).astype(np.float32)
    near, far = np.maximum(near, np.float32(RC.RAY_START)), np.minimum(far, np.float32(RC.RAY_END))
    assert (near < far).all()
    return near, far


@contextlib.contextmanager
def per_ray_depths(near, far):
    """Inside, the ray oracle of render_rays_common (ray_oracle, oracle_run) takes its coarse depths from the per-ray bounds."""
    keep = RC.ray_depths

    def depths(u_strat, S, ray_start, ray_end):
        return torch.from_numpy(bounded_depths(u_strat.float().numpy(), S, near, far))
    RC.ray_depths = depths
    try:
        yield
    finally:
        RC.ray_depths = keep
