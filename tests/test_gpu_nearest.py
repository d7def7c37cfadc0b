"""Nearest points on the GPU: cnerf_nearest_points (through ops.nearest_points and through ctypes) against its NumPy statement
(tests/nearest_common.py), bit for bit on both outputs; shape_metrics.chamfer_distance / f_score values and gradients against float64
on the oracle's outputs; sample_surface and reconstruction_metrics end to end.

Shapes come from the kernel's own constants (cnerf_nearest_points_tiling): Q queries per block, T targets per tile.  Every case is a few
hundred to a few thousand points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import isosurface_common as IC
import nearest_common as NC

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL_D, SENTINEL_J = 12345.0, -77
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def QT():
    from cnerf_amd import _lib as L
    q, t = C.c_int32(0), C.c_int32(0)
    L.check(L.lib().cnerf_nearest_points_tiling(C.byref(q), C.byref(t)), "tiling")
    assert q.value > 1 and t.value > 1
    return q.value, t.value


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def gpu_nearest(dev, q, t, nq=None, mt=None, splits=0):
    from cnerf_amd import ops
    d, j = ops.nearest_points(on(dev, q, F), on(dev, t, F), on(dev, nq, np.int32), on(dev, mt, np.int32), target_splits=splits)
    assert d.dtype == torch.float32 and j.dtype == torch.int32 and d.is_cuda and j.is_cuda
    return d.cpu().numpy(), j.cpu().numpy()


def raw_nearest(dev, q, t, nq=None, mt=None, splits=0):
    """The entry through ctypes with a caller-made workspace and outputs pre-filled with a sentinel."""
    from cnerf_amd import ops, _lib as L
    lib = L.lib()
    B, n, m = q.shape[0], q.shape[1], t.shape[1]
    qd, td, nqd, mtd = on(dev, q, F), on(dev, t, F), on(dev, nq, np.int32), on(dev, mt, np.int32)
    nb = C.c_size_t(0)
    L.check(lib.cnerf_nearest_points_bytes(B, n, m, splits, C.byref(nb)), "bytes")
    ws = torch.full((max(nb.value, 1),), 0xA5, dtype=torch.uint8, device=dev)
    d = torch.full((B, n), SENTINEL_D, dtype=torch.float32, device=dev)
    j = torch.full((B, n), SENTINEL_J, dtype=torch.int32, device=dev)
    L.check(lib.cnerf_nearest_points(B, n, m, L.ptr(qd), L.ptr(td), L.ptr(nqd), L.ptr(mtd), splits, L.ptr(d), L.ptr(j), L.ptr(ws) if nb.value else None,
                                     ops._stream()), "nearest_points")
    return d.cpu().numpy(), j.cpu().numpy(), nb.value


def assert_same(got, want, what):
    assert NC.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]), what


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the oracle, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which_n", range(5))
def test_edges_of_the_tiling(dev, QT, which_n):
    Q, T = QT
    n = (1, Q - 1, Q, Q + 1, 2 * Q + 3)[which_n]
    rng = np.random.default_rng(100 + which_n)
    for m in (1, 2, T - 1, T, T + 1, 3 * T + 5):
        q, t = NC.uniform_cloud(rng, (2, n)), NC.uniform_cloud(rng, (2, m))
        want = NC.nearest(q, t)
        d, j, _ = raw_nearest(dev, q, t, splits=1)
        assert (j != SENTINEL_J).all() and (d != SENTINEL_D).all(), (n, m)       # every element is written
        assert_same((d, j), want, (n, m))
        assert_same(gpu_nearest(dev, q, t), want, (n, m, "auto"))
        assert (want[1] >= 0).all() and (want[1] < m).all()


def tie_clouds(Q, T):
    """Targets drawn with repetition from five positions of the 0.25-lattice, m = 3T + 5, the draw's seed searched (on the CPU) until
    every position occurs in every tile and in every range of 2 and of 3 splits; queries anywhere on the lattice."""
    m, n = 3 * T + 5, 2 * Q + 3
    for seed in range(200):
        rng = np.random.default_rng(seed)
        pool = NC.lattice_cloud(rng, (5,))
        if len(np.unique(pool, axis=0)) < 5:
            continue
        pick = rng.integers(0, 5, (2, m))
        spans = [(k * T, (k + 1) * T) for k in range(3)] + [(r * m // S, (r + 1) * m // S) for S in (2, 3) for r in range(S)]
        if all(len(np.unique(pick[b, lo:hi])) == 5 for b in range(2) for lo, hi in spans):
            return NC.lattice_cloud(rng, (2, n)), pool[pick]
    raise AssertionError("no seed gives every position in every tile and range")


def test_ties_take_the_lowest_index(dev, QT):
    q, t = tie_clouds(*QT)
    want = NC.nearest(q, t)
    d64, j64 = NC.nearest_f64(q, t)
    assert np.array_equal(want[0].astype(np.float64), d64) and np.array_equal(want[1], j64)      # exact arithmetic on this lattice
    for b in range(2):                   # the winner is the first occurrence of its position, which lies in tile 0 and in range 0
        first = {tuple(p): int(np.flatnonzero((t[b] == p).all(1))[0]) for p in np.unique(t[b], axis=0)}
        assert all(first[tuple(t[b, j])] == j for j in want[1][b]) and max(first.values()) < QT[1]
    for splits in (1, 2, 3, 0):
        assert_same(gpu_nearest(dev, q, t, splits=splits), want, splits)


def test_outputs_do_not_depend_on_target_splits(dev, QT):
    Q, T = QT
    rng = np.random.default_rng(7)
    for m in (3 * T + 5, 5, 2500):       # 5: most ranges are empty; 2500: the library's own choice is above 1 for so few queries
        q, t = NC.uniform_cloud(rng, (2, Q + 1)), NC.uniform_cloud(rng, (2, m))
        want = NC.nearest(q, t)
        sizes = {}
        for splits in (0, 1, 2, 3, 7, 64):
            d, j, sizes[splits] = raw_nearest(dev, q, t, splits=splits)
            assert_same((d, j), want, (m, splits))
        assert sizes[1] == 0 and 0 < sizes[2] < sizes[3] < sizes[7] < sizes[64]
        if m == 2500:
            assert sizes[0] > 0


def test_lengths_are_read_on_the_device_and_clamped(dev, QT):
    Q, T = QT
    n, m = Q + 1, 3 * T + 5
    rng = np.random.default_rng(8)
    q, t = NC.uniform_cloud(rng, (3, n)), NC.uniform_cloud(rng, (3, m))
    for nq, mt in (((0, 1, n), (m, 0, T + 1)), ((-5, n + 9, 1), (m + 9, m + 9, -5)), ((n, n, n - 1), (m, m - 1, m))):
        want = NC.nearest(q, t, nq, mt)
        for splits in (1, 3):
            d, j, _ = raw_nearest(dev, q, t, nq, mt, splits=splits)
            assert (j != SENTINEL_J).all() and (d != SENTINEL_D).all()
            assert_same((d, j), want, (nq, mt, splits))
    # the clamp, spelled out: out-of-range lengths give what the clamped ones give
    assert_same(gpu_nearest(dev, q, t, (-5, n + 9, 1), (m + 9, m + 9, -5)), NC.nearest(q, t, (0, n, 1), (m, m, 0)), "clamp")
    d, j = gpu_nearest(dev, q, t, (0, 1, n), (m, 0, T + 1))
    assert np.isinf(d[0]).all() and (j[0] == -1).all() and np.isinf(d[1]).all() and (j[1] == -1).all() and j[2].max() <= T


def test_non_finite_values_are_never_chosen(dev, QT):
    Q, T = QT
    n, m = Q + 1, 3 * T + 5
    rng = np.random.default_rng(9)
    q, t = NC.uniform_cloud(rng, (2, n)), NC.uniform_cloud(rng, (2, m))
    clean = NC.nearest(q, t)
    t[0, clean[1][0, 0]] = np.nan                # the winner of query 0 becomes NaN
    t[0, clean[1][0, 1], 1] = np.inf             # the winner of query 1 becomes infinite
    q[0, 2, 2] = np.nan                          # a NaN query
    q[0, 3, 0] = -np.inf
    q[0, 4], t[0, 5] = F(3e19), F(-3e19)         # finite points whose d overflows against everything
    t[1] = np.nan                                # an image whose targets are all NaN
    want = NC.nearest(q, t)
    assert want[1][0, 0] != clean[1][0, 0] and want[1][0, 0] >= 0 and want[1][0, 1] != clean[1][0, 1]
    assert (want[1][0, 2:5] == -1).all() and np.isinf(want[0][0, 2:5]).all() and not (want[1][0] == 5).any()
    assert (want[1][1] == -1).all() and np.isinf(want[0][1]).all()
    for splits in (1, 3, 64):
        assert_same(gpu_nearest(dev, q, t, splits=splits), want, splits)


def test_other_stream_repeats_and_unbatched_inputs(dev, QT):
    from cnerf_amd import ops, _lib as L
    Q, T = QT
    rng = np.random.default_rng(10)
    q, t = NC.uniform_cloud(rng, (2, Q + 1)), NC.uniform_cloud(rng, (2, 3 * T + 5))
    want = NC.nearest(q, t)
    first = gpu_nearest(dev, q, t, splits=3)
    assert_same(first, want, "first")
    assert_same(gpu_nearest(dev, q, t, splits=3), first, "repeat")
    side = torch.cuda.Stream(device=dev)
    qd, td = on(dev, q, F), on(dev, t, F)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream != torch.cuda.default_stream().cuda_stream
        d, j = ops.nearest_points(qd, td, target_splits=2)
    side.synchronize()
    assert_same((d.cpu().numpy(), j.cpu().numpy()), want, "side stream")
    d1, j1 = ops.nearest_points(qd[1], td[1])                       # (n,3), (m,3): one image, no batch axis in the result
    assert d1.shape == (Q + 1,) and j1.shape == (Q + 1,)
    assert_same((d1.cpu().numpy()[None], j1.cpu().numpy()[None]), (want[0][1:], want[1][1:]), "unbatched")
    # a strided, float64 view that requires grad is detached and made contiguous float32
    wide = torch.zeros(2, Q + 1, 5, dtype=torch.float64, device=dev, requires_grad=True)
    with torch.no_grad():
        wide[..., :3] = qd
    d2, _ = ops.nearest_points(wide[..., :3], td)
    assert not d2.requires_grad and NC.same_bits(d2.cpu().numpy(), want[0])
    for bad_q, bad_t in ((qd[..., :2], td), (qd, td[:1]), (qd[0], td), (qd.reshape(-1), td)):
        with pytest.raises(L.CnerfError):
            ops.nearest_points(bad_q, bad_t)
    with pytest.raises(L.CnerfError):
        ops.nearest_points(qd.cpu(), td.cpu())                      # no CPU fallback
    with pytest.raises(L.CnerfError):
        ops.nearest_points(qd, td, query_lengths=torch.tensor([1, 2, 3]))


# ---------------------------------------------------------------------------------------------------------------------
# 2. chamfer_distance and f_score
# ---------------------------------------------------------------------------------------------------------------------
TAU = 0.1
METRIC_SHAPE = dict(B=3, n=300, m=421, a_len=(300, 257, 0), b_len=(421, 390, 421))


def metric_clouds():
    """Uniform clouds whose seed is searched on the CPU until no oracle distance of a counted row lies within 1e-6 of TAU."""
    s = METRIC_SHAPE
    for seed in range(50):
        rng = np.random.default_rng(1000 + seed)
        a, b = NC.uniform_cloud(rng, (s["B"], s["n"])), NC.uniform_cloud(rng, (s["B"], s["m"]))
        ab, ba = NC.nearest(a, b, s["a_len"], s["b_len"]), NC.nearest(b, a, s["b_len"], s["a_len"])
        if NC.clear_of_threshold(ab[0], TAU) and NC.clear_of_threshold(ba[0], TAU):
            return a, b, ab, ba
    raise AssertionError("no seed keeps every distance clear of tau")


@pytest.fixture(scope="module")
def metric_case():
    return metric_clouds()


def close(got, want, what):
    got, want = float(got), float(want)
    print(f"{what}: got {got!r} want {want!r} rel err {abs(got - want) / abs(want):.3g} (gate {4 * EPS:.3g})")
    assert abs(got - want) <= 4 * EPS * abs(want), what


def test_chamfer_and_f_score_values(dev, metric_case):
    from cnerf_amd import shape_metrics as SM
    s = METRIC_SHAPE
    a, b, ab, ba = metric_case
    assert NC.clear_of_threshold(ab[0], TAU) and NC.clear_of_threshold(ba[0], TAU)
    A, Bc = on(dev, a, F), on(dev, b, F)
    for squared in (True, False):
        got_ab, got_ba = SM.chamfer_distance(A, Bc, s["a_len"], s["b_len"], squared=squared)
        assert got_ab.shape == (3,) and got_ab.dtype == torch.float32
        for i in range(2):
            close(got_ab[i], NC.chamfer_from(ab[0][i], s["a_len"][i], squared), f"a_to_b[{i}] squared={squared}")
            close(got_ba[i], NC.chamfer_from(ba[0][i], s["b_len"][i], squared), f"b_to_a[{i}] squared={squared}")
        assert math.isnan(float(got_ab[2])) and math.isnan(float(got_ba[2]))      # image 2 has an empty side
    f, p, r = SM.f_score(A, Bc, TAU, s["a_len"], s["b_len"])
    for i in range(2):
        wp, wr = NC.share_within(ab[0][i], s["a_len"][i], TAU), NC.share_within(ba[0][i], s["b_len"][i], TAU)
        assert 0 < wp < 1 and 0 < wr < 1                                          # tau separates something
        assert float(p[i]) == F(wp) and float(r[i]) == F(wr) and abs(float(f[i]) - NC.f_from(wp, wr)) <= 2 * EPS
    assert all(math.isnan(float(v[2])) for v in (f, p, r))
    f0, p0, r0 = SM.f_score(A[:1], Bc[:1], 1e-9)                                  # nothing within tau: f = 0, not nan
    assert float(p0) == 0 and float(r0) == 0 and float(f0) == 0
    # unbatched inputs: 0-dim results, the same numbers
    one_ab, one_ba = SM.chamfer_distance(A[0], Bc[0])
    full_ab, full_ba = SM.chamfer_distance(A[:1], Bc[:1])
    assert one_ab.dim() == 0 and float(one_ab) == float(full_ab[0]) and float(one_ba) == float(full_ba[0])


def test_chamfer_gradients(dev, metric_case):
    """Against float64 autograd on the CPU through gather with the oracle's indices.  Per component the gate is (c + 3) 2^-23 times the
    largest addend, c the number of queries that chose the point as their target (from the oracle)."""
    from cnerf_amd import shape_metrics as SM
    s = METRIC_SHAPE
    a, b, ab, ba = metric_case
    w_ab, w_ba = (0.7, 1.3, 0.4), (1.1, 0.6, 2.0)
    A, Bc = on(dev, a, F).requires_grad_(), on(dev, b, F).requires_grad_()
    got_ab, got_ba = SM.chamfer_distance(A, Bc, s["a_len"], s["b_len"])
    loss = torch.nansum(got_ab * torch.tensor(w_ab, device=dev)) + torch.nansum(got_ba * torch.tensor(w_ba, device=dev))
    loss.backward()
    gA, gB = A.grad.cpu().numpy(), Bc.grad.cpu().numpy()
    assert math.isnan(float(got_ab[2].detach())) and not gA[2].any() and not gB[2].any()      # the empty side: nan value, zero gradient
    assert not gA[1, s["a_len"][1]:].any() and not gB[1, s["b_len"][1]:].any()       # rows beyond the lengths take no part
    a64, b64 = torch.from_numpy(a).double().requires_grad_(), torch.from_numpy(b).double().requires_grad_()
    ref = 0
    for i in range(2):
        na, nb = s["a_len"][i], s["b_len"][i]
        j_ab, j_ba = torch.from_numpy(ab[1][i, :na]).long(), torch.from_numpy(ba[1][i, :nb]).long()
        ref = ref + w_ab[i] * ((a64[i, :na] - b64[i][j_ab]) ** 2).sum(-1).mean() + w_ba[i] * ((b64[i, :nb] - a64[i][j_ba]) ** 2).sum(-1).mean()
    ref.backward()
    for i in range(2):
        na, nb = s["a_len"][i], s["b_len"][i]
        for name, got, want, x, y, nx, ny, jx, jy, wx, wy in (("a", gA[i], a64.grad[i].numpy(), a[i], b[i], na, nb, ab[1][i], ba[1][i], w_ab[i], w_ba[i]),
                                                              ("b", gB[i], b64.grad[i].numpy(), b[i], a[i], nb, na, ba[1][i], ab[1][i], w_ba[i], w_ab[i])):
            x, y = x.astype(np.float64), y.astype(np.float64)
            addend = np.zeros_like(x)
            addend[:nx] = np.abs(2 * wx / nx * (x[:nx] - y[jx[:nx]]))                    # as a query
            back = np.abs(2 * wy / ny * (y[:ny] - x[jy[:ny]]))                           # as the target of y's queries
            np.maximum.at(addend, jy[:ny], back)
            c = np.bincount(jy[:ny], minlength=len(x))
            gate = (c[:, None] + 3) * EPS * addend
            err = np.abs(got - want)
            print(f"grad {name}[{i}]: max err / gate {np.max(err[gate > 0] / gate[gate > 0]):.3g}, most choosers {c.max()}")
            assert (err <= gate).all() and c.max() >= 3


# ---------------------------------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------------------------------
def clear_tau(dists, share=0.5):
    """A threshold in the middle of the widest gap among the sorted distances around the given quantile: no distance is near it."""
    d = np.sort(np.concatenate([np.sqrt(np.asarray(x, np.float64)).ravel() for x in dists]))
    k = int(share * len(d))
    window = d[max(k - 50, 0):k + 50]
    g = int(np.argmax(np.diff(window)))
    return float((window[g] + window[g + 1]) / 2)


def check_metrics_against_the_oracle(samples, cloud, tau, got):
    """got: chamfer a_to_b, b_to_a, f, precision, recall as floats, computed on the device for (samples, cloud)."""
    s, c = samples[None].astype(F), cloud[None].astype(F)
    ab, ba = NC.nearest(s, c), NC.nearest(c, s)
    assert NC.clear_of_threshold(ab[0], tau) and NC.clear_of_threshold(ba[0], tau)
    close(got[0], NC.chamfer_from(ab[0][0], len(samples)), "mesh to cloud")
    close(got[1], NC.chamfer_from(ba[0][0], len(cloud)), "cloud to mesh")
    wp, wr = NC.share_within(ab[0][0], len(samples), tau), NC.share_within(ba[0][0], len(cloud), tau)
    assert 0 < wp < 1 and 0 < wr < 1
    assert got[3] == F(wp) and got[4] == F(wr) and abs(got[2] - NC.f_from(wp, wr)) <= 2 * EPS


def test_ball_mesh_samples_and_metrics(dev):
    from cnerf_amd import ops, shape_metrics as SM
    ball = NC.BALL
    values = IC.ball_field(ball["shape"], [ball["center"]], ball["radius"], ball["lo"], ball["pitch"])
    v, f, _ = ops.isosurface(on(dev, values, F), 0.0, lo=ball["lo"], pitch=ball["pitch"])
    u = on(dev, NC.fixed_u(4096, 21), F)
    points, face_idx, bary = SM.sample_surface(v, f, 4096, u=u)
    assert points.is_cuda and points.shape == (4096, 3) and int(face_idx.max()) < len(f)
    P = points.cpu().numpy()
    off = np.abs(np.linalg.norm(P.astype(np.float64) - np.asarray(ball["center"]), axis=1) - ball["radius"])
    print("ball samples: max | |p - c| - r | =", off.max(), "pitch", ball["pitch"])
    assert off.max() <= ball["pitch"]                       # tests/test_nearest_cpu.py verifies this bound with the isosurface oracle
    want = (bary.cpu().numpy().astype(np.float64)[:, :, None] * v.cpu().numpy()[f.cpu().numpy()[face_idx.cpu().numpy()]].astype(np.float64)).sum(1)
    assert np.abs(P - want).max() <= 4 * EPS * np.abs(v.cpu().numpy()).max()
    cloud = NC.sphere_cloud(3000, 22, ball["center"], ball["radius"])
    Cd = on(dev, cloud, F)
    d_ab, d_ba = NC.nearest(P[None], cloud[None]), NC.nearest(cloud[None], P[None])
    tau = clear_tau((d_ab[0], d_ba[0]))
    ab, ba = SM.chamfer_distance(points, Cd)
    fs, p, r = SM.f_score(points, Cd, tau)
    check_metrics_against_the_oracle(P, cloud, tau, tuple(float(x) for x in (ab, ba, fs, p, r)))
    assert float(ab) <= ball["pitch"] ** 2 * 4              # the cloud is on the sphere, about 0.05 apart: the mesh hugs it


def test_reconstruction_metrics_end_to_end(dev):
    from cnerf_amd import extract_shapes as X, shape_metrics as SM
    from cnerf_amd.generators import ImplicitGenerator3d
    torch.manual_seed(11)
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 32, 32, 4, 64).to(dev)
    gen.set_device(dev)
    z = (torch.randn(1, 32, 8, 8, 8, device=dev), torch.randn(1, 32, device=dev))
    N, n_samples = 16, 2048
    sigma = X.sample_generator(gen, z, voxel_resolution=N)
    level = float(np.median(sigma))
    rng = np.random.default_rng(23)
    cloud = np.concatenate([rng.uniform(-0.6, 0.6, (1500, 3)), rng.uniform(0, 1, (1500, 3))], 1).astype(F)      # xyz and three colour columns
    u = NC.fixed_u(n_samples, 24)
    kw = dict(voxel_resolution=N, level=level, n_samples=n_samples, u=torch.from_numpy(u), return_samples=True)
    _, samples = SM.reconstruction_metrics(gen, z, torch.from_numpy(cloud), tau=0.05, **kw)
    S = samples.cpu().numpy()
    assert samples.is_cuda and S.shape == (n_samples, 3) and np.abs(S).max() <= 0.6 + 1e-6
    xyz = np.ascontiguousarray(cloud[:, :3])
    tau = clear_tau((NC.nearest(S[None], xyz[None])[0], NC.nearest(xyz[None], S[None])[0]))
    out, again = SM.reconstruction_metrics(gen, z, torch.from_numpy(cloud)[None], tau=tau, **kw)       # (1,N,6) this time
    assert torch.equal(again, samples)
    v, f, _ = X.extract_mesh(gen, z, voxel_resolution=N, level=level, colors=False)
    assert out["vertices"] == len(v) > 0 and out["triangles"] == len(f) > 0
    assert all(isinstance(out[k], float) for k in SM.METRIC_KEYS) and isinstance(out["vertices"], int)
    check_metrics_against_the_oracle(S, xyz, tau, (out["chamfer_mesh_to_cloud"], out["chamfer_cloud_to_mesh"], out["f_score"], out["precision"],
                                                   out["recall"]))
    assert out["chamfer"] == out["chamfer_mesh_to_cloud"] + out["chamfer_cloud_to_mesh"]
    kw["level"] = float(sigma.max()) + 1.0                          # above every value: no surface
    empty, none = SM.reconstruction_metrics(gen, z, torch.from_numpy(cloud), tau=tau, **kw)
    assert empty["vertices"] == 0 and empty["triangles"] == 0 and none.shape == (0, 3)
    assert all(math.isnan(empty[k]) for k in SM.METRIC_KEYS)
