"""Nearest points: the contract of cnerf_nearest_points (include/cnerf.h) restated in NumPy float32, the same formulas the metrics of
shape_metrics.py are made of in float64, and the clouds the tests share.  No GPU, no torch."""
import numpy as np

F = np.float32
INF = F(np.inf)


def nearest(queries, targets, n_queries=None, n_targets=None, chunk=2048):
    """queries (B,n,3), targets (B,m,3) float32; n_queries / n_targets (B,) or None -> dist2 (B,n) float32, idx (B,n) int32.

    d = (dx*dx + dy*dy) + dz*dz with dx = qx - tx ..., every operation a float32 operation of its own (NumPy array arithmetic never
    contracts).  A d that is NaN or +inf is masked to +inf; argmin returns the FIRST minimum, the lowest index; idx = -1 and
    dist2 = +inf where the minimum is +inf.  Lengths are clamped to [0,n] / [0,m]; rows at or beyond the query length are (+inf, -1).
    Chunked over targets: a later chunk replaces the running best only where it is strictly below, which keeps the lowest index."""
    q, t = np.ascontiguousarray(queries, F), np.ascontiguousarray(targets, F)
    B, n, m = q.shape[0], q.shape[1], t.shape[1]
    dist2 = np.full((B, n), INF, F)
    idx = np.full((B, n), -1, np.int32)
    for b in range(B):
        nq = n if n_queries is None else int(np.clip(int(n_queries[b]), 0, n))
        mt = m if n_targets is None else int(np.clip(int(n_targets[b]), 0, m))
        if nq == 0:
            continue
        best, bj = np.full(nq, INF, F), np.full(nq, -1, np.int64)
        for j0 in range(0, mt, chunk):
            tc = t[b, j0:min(j0 + chunk, mt)]
            with np.errstate(over="ignore", invalid="ignore"):
                dx = q[b, :nq, None, 0] - tc[None, :, 0]
                dy = q[b, :nq, None, 1] - tc[None, :, 1]
                dz = q[b, :nq, None, 2] - tc[None, :, 2]
                d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == F
            d = np.where(np.isfinite(d), d, INF)
            k = np.argmin(d, axis=1)
            dk = d[np.arange(nq), k]
            take = dk < best
            best = np.where(take, dk, best)
            bj = np.where(take, k + j0, bj)
        dist2[b, :nq] = best
        idx[b, :nq] = np.where(best < INF, bj, -1)
    return dist2, idx


def nearest_f64(queries, targets):
    """Float64 brute force without any special case, for clouds on which float32 arithmetic is exact: dist2 (B,n) float64, idx (B,n)."""
    q, t = np.asarray(queries, np.float64), np.asarray(targets, np.float64)
    d = ((q[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1)
    k = np.argmin(d, axis=2)
    return np.take_along_axis(d, k[..., None], 2)[..., 0], k.astype(np.int32)


def uniform_cloud(rng, shape):
    return rng.uniform(-1.0, 1.0, tuple(shape) + (3,)).astype(F)


def lattice_cloud(rng, shape):
    """Coordinates that are multiples of 0.25 in [-1, 1] (9 values per axis, 729 positions): differences, squares and their sums are
    exact in float32, so distances tie exactly and positions recur."""
    return (rng.integers(-4, 5, tuple(shape) + (3,)) * 0.25).astype(F)


def fixed_u(n, seed):
    """(n,3) float32 in [0,1): the numbers sample_surface draws with."""
    return np.minimum(np.random.default_rng(seed).random((n, 3)).astype(F), F(1 - 2.0 ** -24))


def sphere_cloud(n, seed, center, radius):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (np.asarray(center) + radius * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F)


# an analytic ball on a 24^3 lattice (isosurface_common.ball_field): the mesh the end-to-end tests sample
BALL = dict(shape=(24, 24, 24), lo=(-1.1, -1.0, -1.2), pitch=0.1, center=(0.05, 0.1, -0.07), radius=0.83)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the metrics' formulas on the oracle's outputs, float64 ----------------------------------------------------------------------------
def chamfer_from(dist2, n_valid, squared=True):
    """Mean over the first n_valid rows of one image's dist2 (float64; the root first when not squared)."""
    d = np.asarray(dist2, np.float64)[:n_valid]
    return float(np.mean(d if squared else np.sqrt(d)))


def share_within(dist2, n_valid, tau):
    d = np.sqrt(np.asarray(dist2, np.float64)[:n_valid])
    return float(np.count_nonzero(d <= tau)) / n_valid


def f_from(p, r):
    return 2 * p * r / (p + r) if p + r > 0 else 0.0


def clear_of_threshold(dist2, tau, margin=1e-6):
    """No distance within `margin` of tau: the F-score's counts cannot depend on the last bits of a root."""
    d = np.sqrt(np.asarray(dist2, np.float64))
    d = d[np.isfinite(d)]
    return bool(np.all(np.abs(d - tau) > margin))
