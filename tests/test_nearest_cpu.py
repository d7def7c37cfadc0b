"""Nearest points and shape metrics, no GPU: the host code's exports, workspace sizes, tiling constants and refusals; the NumPy statement
of the contract (tests/nearest_common.py) against a float64 brute force where float32 is exact; shape_metrics.sample_surface on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import nearest_common as NC

ENTRIES = ("cnerf_nearest_points_tiling", "cnerf_nearest_points_bytes", "cnerf_nearest_points")
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
    import cnerf_amd
    assert cnerf_amd.shape_metrics.chamfer_distance and callable(cnerf_amd.ops.nearest_points)


def test_tiling_is_positive(L):
    q, t = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.lib().cnerf_nearest_points_tiling(ctypes.byref(q), ctypes.byref(t)) == 0
    assert q.value > 0 and t.value > 0
    assert L.lib().cnerf_nearest_points_tiling(None, None) == 0


def test_workspace_is_zero_for_one_range_and_grows_with_splits_images_and_queries(L):
    lib = L.lib()
    nb = ctypes.c_size_t(7)

    def size(B, n, m, s):
        assert lib.cnerf_nearest_points_bytes(B, n, m, s, ctypes.byref(nb)) == 0, lib.cnerf_last_error()
        return nb.value

    for B, n, m in ((1, 1, 1), (3, 1000, 5), (2, 100_000, 1_000_000)):
        assert size(B, n, m, 1) == 0
    base = size(2, 1000, 5000, 2)
    assert base >= 8 * 2 * 2 * 1000                                  # a float and an int32 per (image, range, query)
    assert size(2, 1000, 5000, 4) > base and size(4, 1000, 5000, 2) > base and size(2, 2000, 5000, 2) > base
    assert size(2, 1000, 5000, 1024) >= 8 * 1024 * 2 * 1000
    assert size(2, 1000, 9000, 2) == base                            # not with the targets
    # the library's own choice is a pure function of (B, n, m): asked twice, the same answer; few queries against many targets split
    assert size(1, 2048, 1_000_000, 0) == size(1, 2048, 1_000_000, 0) > 0
    assert lib.cnerf_nearest_points_bytes(1, 5, 5, 0, None) == 0      # the size pointer is optional


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t()

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def call(B=2, n=100, m=200, queries=fake, targets=fake, nq=None, mt=None, splits=1, dist2=fake, idx=fake, ws=None):
        return lib.cnerf_nearest_points(B, n, m, queries, targets, nq, mt, splits, dist2, idx, ws, None)

    for kw, word in ((dict(B=0), "B=0"), (dict(B=-1), "B=-1"), (dict(n=0), "n=0"), (dict(n=-4), "n=-4"), (dict(m=0), "m=0"), (dict(m=-1), "m=-1"),
                     (dict(m=2 ** 31), "2^31"), (dict(B=1, n=2 ** 40), "2^40"), (dict(B=1024, n=2 ** 30), "2^40"), (dict(splits=-1), "target_splits=-1"),
                     (dict(splits=1025), "target_splits=1025")):
        refused(call(**kw), word)
        shape = dict(B=2, n=100, m=200, splits=1)
        shape.update(kw)
        refused(lib.cnerf_nearest_points_bytes(shape["B"], shape["n"], shape["m"], shape["splits"], ctypes.byref(nb)), word)
    assert lib.cnerf_nearest_points_bytes(1, 2 ** 40 - 1, 2 ** 31 - 1, 1, ctypes.byref(nb)) == 0      # the largest shapes that pass
    assert lib.cnerf_nearest_points_bytes(1024, 2 ** 30 - 1, 1, 1024, ctypes.byref(nb)) == 0
    for missing in ("queries", "targets", "dist2", "idx"):
        refused(call(**{missing: None}), "NULL")
    refused(call(splits=2, ws=None), "workspace")
    refused(call(n=2048, m=1_000_000, B=1, splits=0, ws=None), "workspace")       # the library's own choice needs one here


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_float64_brute_force_on_the_quarter_lattice():
    """Coordinates are multiples of 0.25 in [-1, 1]: every float32 operation of the contract is exact, so distances, indices and the
    lowest-index tie rule must agree exactly with a float64 brute force; chunking over targets must not show."""
    rng = np.random.default_rng(0)
    q, t = NC.lattice_cloud(rng, (2, 300)), NC.lattice_cloud(rng, (2, 1500))
    want_d, want_j = NC.nearest_f64(q, t)
    for chunk in (2048, 64, 7):
        d, j = NC.nearest(q, t, chunk=chunk)
        assert d.dtype == F and j.dtype == np.int32
        assert np.array_equal(d.astype(np.float64), want_d) and np.array_equal(j, want_j)
    assert (want_d == 0).mean() > 0.5                               # 729 positions, 1500 targets: most queries sit on a target ...
    first = np.array([[np.flatnonzero((t[b] == q[b, i]).all(1))[0] if want_d[b, i] == 0 else -1 for i in range(300)] for b in range(2)])
    assert np.array_equal(first[want_d == 0], want_j[want_d == 0])   # ... and take its first occurrence


def test_oracle_lengths_and_non_finite_values():
    rng = np.random.default_rng(1)
    q, t = NC.uniform_cloud(rng, (3, 40)), NC.uniform_cloud(rng, (3, 90))
    full_d, full_j = NC.nearest(q, t)
    d, j = NC.nearest(q, t, n_queries=(0, 1, 99), n_targets=(90, 0, -3))
    assert np.isinf(d[0]).all() and (j[0] == -1).all()                                  # no query counts
    assert np.isinf(d[1]).all() and (j[1] == -1).all()                                  # no target counts
    assert np.isinf(d[2]).all() and (j[2] == -1).all()                                  # -3 clamps to 0 targets, 99 to 40 queries
    d, j = NC.nearest(q, t, n_queries=(40, 7, 40), n_targets=(33, 90, 500))
    assert np.array_equal(d[2], full_d[2]) and np.array_equal(j[2], full_j[2]) and j[0].max() < 33
    assert np.array_equal(d[1, :7], full_d[1, :7]) and np.isinf(d[1, 7:]).all() and (j[1, 7:] == -1).all()
    t2, q2 = t.copy(), q.copy()
    t2[0, full_j[0, 0]] = np.nan                                    # the winner of query 0 disappears
    t2[0, full_j[0, 1], 1] = np.inf
    q2[0, 2, 2] = np.nan
    q2[0, 3], t2[0, 5] = F(3e19), F(-3e19)                          # overflows against everything
    t2[1] = np.nan
    d, j = NC.nearest(q2, t2)
    assert j[0, 0] != full_j[0, 0] and j[0, 0] >= 0 and d[0, 0] >= full_d[0, 0] and j[0, 1] != full_j[0, 1]
    assert np.isinf(d[0, 2]) and j[0, 2] == -1 and np.isinf(d[0, 3]) and j[0, 3] == -1 and not (j[0] == 5).any()
    assert np.isinf(d[1]).all() and (j[1] == -1).all()
    assert np.array_equal(d[2], full_d[2]) and np.array_equal(j[2], full_j[2])


# ---------------------------------------------------------------------------------------------------------------------
# sample_surface on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def two_triangles():
    """Areas 1, 0, 3 in that order: a right triangle with legs 1 and 2, a degenerate one (two equal corners), a right triangle with
    legs 2 and 3 elsewhere.  Coordinates up to 7 in magnitude."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0],
                  [5, 5, 5],
                  [-7, 1, 2], [-7, 3, 2], [-7, 1, 5]], F)
    f = np.array([[0, 1, 2], [3, 3, 0], [4, 5, 6]], np.int64)
    return v, f


def test_sample_surface_counts_barycentrics_and_attributes(L):
    from cnerf_amd import shape_metrics as SM
    v, f = two_triangles()
    n = 4096
    rng = np.random.default_rng(5)
    u = np.stack([(rng.permutation(n) + 0.5) / n, rng.random(n), rng.random(n)], 1).astype(F)
    u0 = u[:, 0].astype(np.float64)
    assert np.abs(u0 - 0.25).min() >= 1 / 8192 - 1e-12 and u.max() < 1            # no draw near the boundary between the two triangles
    attrs = rng.standard_normal((len(v), 4)).astype(F)
    points, face_idx, bary, a = SM.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u=torch.from_numpy(u), attrs=torch.from_numpy(attrs))
    assert points.shape == (n, 3) and face_idx.shape == (n,) and bary.shape == (n, 3) and a.shape == (n, 4)
    assert points.dtype == torch.float32 and bary.dtype == torch.float32 and face_idx.dtype == torch.int64
    points, face_idx, bary, a = points.numpy(), face_idx.numpy(), bary.numpy(), a.numpy()
    counts = np.bincount(face_idx, minlength=3)
    assert counts.tolist() == [1024, 0, 3072]
    assert np.array_equal(face_idx, np.where(u0 < 0.25, 0, 2))
    b64 = bary.astype(np.float64)
    assert (bary >= 0).all() and np.abs(b64.sum(1) - 1).max() <= 2.0 ** -22
    s, u2 = np.sqrt(u[:, 1].astype(np.float64)), u[:, 2].astype(np.float64)      # the formula itself, in float64: three fp32 roundings away
    assert np.abs(b64 - np.stack([1 - s, s * (1 - u2), s * u2], 1)).max() <= 2.0 ** -22
    for got, values in ((points, v), (a, attrs)):
        want = (b64[:, :, None] * values[f[face_idx]].astype(np.float64)).sum(1)
        err = np.abs(got - want).max()
        print("sample_surface max|err|", err, "bound", 4 * 2.0 ** -23 * np.abs(values).max())
        assert err <= 4 * 2.0 ** -23 * np.abs(values).max()
    # each in the plane of its triangle: z = 0 exactly (all three addends are 0), x = -7 as far as the weights sum to 1
    assert (points[face_idx == 0, 2] == 0).all() and np.abs(points[face_idx == 2, 0] + 7).max() <= 4 * 2.0 ** -23 * 7
    # without attrs: three results, the same draw
    p3 = SM.sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, u=torch.from_numpy(u))
    assert len(p3) == 3 and np.array_equal(p3[0].numpy(), points)


def test_ball_samples_lie_within_one_pitch_of_the_sphere(L):
    """The bound tests/test_gpu_nearest.py relies on, verified with the isosurface oracle: area-weighted samples of the marching-
    tetrahedra mesh of an analytic ball keep within one lattice pitch of the sphere (they are in fact far closer: chords of a sphere
    of radius 8.3 pitches)."""
    import isosurface_common as IC
    from cnerf_amd import shape_metrics as SM
    ball = NC.BALL
    values = IC.ball_field(ball["shape"], [ball["center"]], ball["radius"], ball["lo"], ball["pitch"])
    verts, faces, _ = IC.isosurface(values, 0.0, ball["lo"], ball["pitch"])
    assert IC.edge_census(faces) == (1, 0) and IC.euler_characteristic(len(verts), faces) == 2
    points, face_idx, _ = SM.sample_surface(torch.from_numpy(verts), torch.from_numpy(faces.astype(np.int64)), 4096, u=torch.from_numpy(NC.fixed_u(4096, 21)))
    off = np.abs(np.linalg.norm(points.numpy().astype(np.float64) - np.asarray(ball["center"]), axis=1) - ball["radius"])
    print("max | |p - c| - r | =", off.max(), "pitch", ball["pitch"])
    assert off.max() <= ball["pitch"]
    area = np.linalg.norm(IC.normals(verts, faces), axis=1) / 2
    assert (area[face_idx.numpy()] > 0).all() and abs(area.sum() / (4 * np.pi * ball["radius"] ** 2) - 1) < 0.02


def test_sample_surface_random_draws_and_refusals(L):
    from cnerf_amd import shape_metrics as SM
    v, f = (torch.from_numpy(x) for x in two_triangles())
    g = torch.Generator().manual_seed(3)
    p1, k1, _ = SM.sample_surface(v, f, 2000, generator=g)
    p2, k2, _ = SM.sample_surface(v, f, 2000, generator=torch.Generator().manual_seed(3))
    assert torch.equal(p1, p2) and torch.equal(k1, k2) and (k1 != 1).all()
    share = (k1 == 2).float().mean().item()
    assert abs(share - 0.75) < 5 * (0.75 * 0.25 / 2000) ** 0.5                     # five standard deviations of a binomial share
    # a trailing zero-area triangle is never drawn either, even by the largest u0
    f2 = torch.cat([f, torch.tensor([[3, 3, 3]])])
    u = torch.tensor([[1 - 2.0 ** -24, 0.3, 0.3], [0.0, 0.3, 0.3]])
    assert SM.sample_surface(v, f2, 2, u=u)[1].tolist() == [2, 0]
    with pytest.raises(ValueError):
        SM.sample_surface(v, torch.tensor([[3, 3, 0]]), 4)
    with pytest.raises(ValueError):
        SM.sample_surface(v, f, 4, u=torch.zeros(5, 3))
    with pytest.raises(ValueError):
        SM.sample_surface(v, f[:, :2], 4)
