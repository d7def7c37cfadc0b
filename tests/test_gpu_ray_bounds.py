"""Per-ray sampling bounds on the GPU: cnerf_occupancy_ray_bounds against hand values and against the float64 statement of its contract
(tests/ray_bounds_common.py), the per-ray coarse sampler against the scalar one, NumPy float32 and the ray oracle, the backward of a
bounded render against float64 autograd, and the public interface end to end (build_occupancy -> ray_bounds -> render_rays).

Shapes: traversal -- G in {4, 8, 12}, two cubes with an asymmetric corner (side 2 and 1.5: a cell edge that is and is not a power of two),
B = 2 with a different bit pattern per image, 203 random unnormalised rays and ten hand-made ones per image (213 rays: three full waves and
a ragged one).  Renders -- B = 2, P = 37 or 19 rays, S in {2, 12, 128}, H = 64, V = 8.

Gates: traversal exact (==) where every depth is representable, else the sandwich of ray_bounds_common with delta = 32 * 2^-23 * M
(derived at delta_of; tests/test_ray_bounds_cpu.py shows that the float64 reference on inputs moved by one float32 ulp stays inside it);
sampler bit for bit; renders and gradients with the gates of tests/test_gpu_render_rays.py and tests/test_gpu_occupancy.py."""
import numpy as np
import pytest
import torch

import occupancy_common as OC
import ray_bounds_common as BC
import render_rays_common as RC
from conftest import scaled_err
from oracle.checks import rgb_sigma_err
from test_gpu_occupancy import COMPOSITE_TOL, check_pass, grid_of, oracle_image
from test_gpu_render_rays import TOL, on_device, rel_l2, upstream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def device_grid(cells, lo, side, G, dev):
    from cnerf_amd import ops
    words = OC.pack_bits(np.asarray(cells, bool).reshape(len(cells), -1))
    return ops.OccupancyGrid(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev), tuple(float(v) for v in lo), float(side), G)


def device_bounds(grid, origins, dirs, t_min, t_max, pad, dev):
    from cnerf_amd import ops
    near, far, hit = ops.occupancy_ray_bounds(grid, torch.from_numpy(origins).to(dev), torch.from_numpy(dirs).to(dev), t_min, t_max, pad)
    assert near.dtype == torch.float32 and far.dtype == torch.float32 and hit.dtype == torch.uint8
    assert near.shape == origins.shape[:2] and far.shape == near.shape and hit.shape == near.shape
    return near.cpu().numpy(), far.cpu().numpy(), hit.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the traversal
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_cases_equal_the_hand_values(dev):
    """lo = -1, side = 2, G = 8: origins on multiples of 1/32, directions +-1, +-2, +-0.5 or +-0.0 per component -- every plane, difference
    and quotient is representable, so near, far and hit are the hand values of ray_bounds_common.exact_cases, with ==; pad 0 and 1/8."""
    o, d, cells, want = BC.exact_cases()
    grid = device_grid(cells, [-1.0] * 3, 2.0, 8, dev)
    o2, d2 = np.ascontiguousarray(np.broadcast_to(o, (2, *o.shape))), np.ascontiguousarray(np.broadcast_to(d, (2, *d.shape)))
    assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()             # both zeros
    for pad, (w_near, w_far, w_hit) in want.items():
        near, far, hit = device_bounds(grid, o2, d2, BC.EXACT_T_MIN, BC.EXACT_T_MAX, pad, dev)
        assert np.array_equal(hit, w_hit.astype(np.uint8)), (pad, hit, w_hit)
        assert np.array_equal(near, w_near.astype(np.float32)), (pad, near, w_near)
        assert np.array_equal(far, w_far.astype(np.float32)), (pad, far, w_far)
    # two runs agree bit for bit
    again = device_bounds(grid, o2, d2, BC.EXACT_T_MIN, BC.EXACT_T_MAX, 0.125, dev)
    assert OC.same_bits(again[0], near) and OC.same_bits(again[1], far) and np.array_equal(again[2], hit)


@pytest.mark.parametrize("side", list(BC.CUBES))
@pytest.mark.parametrize("G", [4, 8, 12])
def test_bounds_lie_in_the_float64_sandwich(dev, G, side):
    """pad = 0.  Omega- / Omega+ = every set cell shrunk / grown by delta; where hit is set hull(T(Omega-)) in [near, far] in
    hull(T(Omega+)); hit = 1 where T(Omega-) is not empty, 0 where T(Omega+) is empty, either in between -- so no grazing ray is excluded
    by hand and every ray is compared.  delta = 32 * 2^-23 * M, M the largest coordinate magnitude among origins and cube corners: four
    roundings each in a crossing depth and in a position, times four (ray_bounds_common.delta_of); a distance in space, whose room in t
    scales with 1 / |d_k| exactly as the rounding error of (plane - o_k) / d_k does."""
    lo = BC.CUBES[side]
    origins, dirs = BC.sandwich_rays(lo, side, 100 * G + int(side * 10))
    P = origins.shape[1]
    assert P == 213
    hits = misses = 0
    for kinds in (("clear", "set"), ("ball", "sparse"), ("sparse", "ball")):
        cells = [BC.pattern_cells(k, G, seed=G + b) for b, k in enumerate(kinds)]
        near, far, hit = device_bounds(device_grid(cells, lo, side, G, dev), origins, dirs, BC.T_MIN, BC.T_MAX, 0.0, dev)
        assert np.isin(hit, (0, 1)).all() and np.isfinite(near).all() and np.isfinite(far).all()
        for b in range(2):
            delta = BC.delta_of(origins[b], lo, side)
            inner, outer = BC.sandwich(origins[b], dirs[b], cells[b], lo, side, G, BC.T_MIN, BC.T_MAX, delta)
            bad = BC.sandwich_violations(near[b], far[b], hit[b], inner, outer, BC.T_MIN, BC.T_MAX)
            assert not bad, (kinds[b], G, side, delta, [(r, why, origins[b, r].tolist(), dirs[b, r].tolist()) for r, why in bad[:4]])
            if kinds[b] == "clear":
                assert not hit[b].any()
            hits, misses = hits + int(hit[b].sum()), misses + int((hit[b] == 0).sum())
    print(f"G={G} side={side}: {hits} hits, {misses} misses")
    assert hits > 300 and misses > 250


def test_padded_bounds_hold_every_live_probe(dev):
    """pad = a quarter cell edge: of 512 depths per ray over [t_min, t_max], every one whose float32 position (o + d t: RC.numpy_points)
    is inside the cube and in a set cell by occupancy_common's rule satisfies near <= t <= far, with no slack, and its ray has hit = 1."""
    G, side = 8, 1.5
    lo = BC.CUBES[side]
    origins, dirs = BC.sandwich_rays(lo, side, 77)
    cells = [BC.pattern_cells("ball", G), BC.pattern_cells("sparse", G, seed=3)]
    words = OC.pack_bits(np.stack(cells))
    pad = 0.25 * side / G
    near, far, hit = device_bounds(device_grid(cells, lo, side, G, dev), origins, dirs, BC.T_MIN, BC.T_MAX, pad, dev)
    t = np.linspace(BC.T_MIN, BC.T_MAX, 512).astype(np.float32)
    t[0], t[-1] = np.float32(BC.T_MIN), np.float32(BC.T_MAX)
    z = np.ascontiguousarray(np.broadcast_to(t, (*origins.shape[:2], 512)))
    pts = RC.numpy_points(origins, dirs, z)
    qualifying = 0
    for b in range(2):
        idx = OC.cell_index(pts[b].reshape(-1, 3), lo, side, G)
        q = ((idx >= 0) & OC.bit_at(words[b], np.maximum(idx, 0))).reshape(-1, 512)
        assert (hit[b][q.any(1)] == 1).all()
        ok = (near[b][:, None] <= z[b]) & (z[b] <= far[b][:, None])
        assert ok[q].all(), (b, np.argwhere(q & ~ok)[:5])
        qualifying += int(q.sum())
        # and the padded interval is not the whole one: the bounds say something
        assert ((far[b] - near[b])[hit[b] == 1] < 0.8 * (BC.T_MAX - BC.T_MIN)).any()
    assert qualifying > 5000


# ---------------------------------------------------------------------------------------------------------------------
# 2. the per-ray sampler
# ---------------------------------------------------------------------------------------------------------------------
def render(case, dev, rng, near=None, far=None, occupancy=None, requires_grad=False):
    """gen.render_rays -> (pixels, dist, aux, leaves); near / far NumPy (B,P) or tensors."""
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(requires_grad)
    vols, glob, o, d = [leaf(v) for v in case.vols], leaf(case.glob), leaf(case.origins), leaf(case.dirs)
    kw = {}
    if near is not None:
        as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        kw.update(ray_near=as_t(near), ray_far=as_t(far))
    if occupancy is not None:
        kw["occupancy"] = occupancy
    aux = {}
    with torch.set_grad_enabled(requires_grad):
        px, dist = case.gen.render_rays(RC.generator_z(case, vols, glob), o, d, RC.RAY_START, RC.RAY_END, case.S, case.hierarchical,
                                        clamp_mode=case.clamp, nerf_noise=case.noise, white_back=case.white_back, last_back=case.last_back,
                                        _rng={k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in rng.items()}, _aux=aux, **kw)
    return px, dist, aux, dict(vols=vols, glob=glob, origins=o, dirs=d)


def assert_same_render(a, b, what):
    (px_a, dist_a, aux_a, _), (px_b, dist_b, aux_b, _) = a, b
    assert OC.same_bits(px_a.cpu().numpy(), px_b.cpu().numpy()) and OC.same_bits(dist_a.cpu().numpy(), dist_b.cpu().numpy()), what
    assert set(aux_a) == set(aux_b) and len(aux_a) >= 4, (what, set(aux_a) ^ set(aux_b))
    for k in aux_a:
        assert torch.equal(aux_a[k].cpu(), aux_b[k].cpu()) if aux_a[k].dtype != torch.float32 else OC.same_bits(aux_a[k].cpu().numpy(), aux_b[k].cpu().numpy()), (what, k)


@pytest.mark.parametrize("draws", ["u_strat", "philox"])
@pytest.mark.parametrize("hier", [True, False])
@pytest.mark.parametrize("S", [2, 12, 128])
def test_full_interval_bounds_are_the_unbounded_call_bit_for_bit(dev, S, hier, draws):
    """near / far filled with ray_start / ray_end: pixels, dist and every aux tensor bit-identical to the call without the keys -- fp32 and
    fp16x3, plain and masked (a ball grid)."""
    B, P = 2, 37
    case = RC.make_case("SHORTSIREN_FG", 64, B, P, S, V=8, seed=S, hierarchical=hier, unnormalised=True)
    on_device(case, dev)
    rng = dict(case.rng) if draws == "u_strat" else {"philox": (0x243F6A8885A308D3, 5)}
    near, far = np.full((B, P), RC.RAY_START, np.float32), np.full((B, P), RC.RAY_END, np.float32)
    grid = grid_of(np.stack([OC.pack_bits(OC.ball_cells(8, 2.5)), OC.pack_bits(OC.ball_cells(8, 3.5))]), dev, 8)
    for prec in ("fp32", "fp16x3"):
        case.gen.siren.precision = prec
        assert_same_render(render(case, dev, rng, near, far), render(case, dev, rng), (prec, "plain"))
        masked = render(case, dev, rng, near, far, occupancy=grid)
        assert_same_render(masked, render(case, dev, rng, occupancy=grid), (prec, "masked"))
        assert 0 < int(masked[2]["live_coarse"].sum()) < B * P * S


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "SHORTSIREN"])
def test_bounded_render_against_numpy_and_the_oracle(dev, variant):
    """Random per-ray bounds, ray_start <= near < far <= ray_end, every fourth span 1 - 2 % of the interval.  coarse_z and coarse_points
    bit-equal to the NumPy float32 statement (a per-ray linspace32), with injected draws and with Philox; pixels, dist and the fine pass
    (forced fine depths: the oracle's) against the ray oracle run on the per-ray depths, at the gate TOL of tests/test_gpu_render_rays.py."""
    B, P, S = 2, 37, 12
    case = RC.make_case(variant, 64, B, P, S, V=8, seed=23, unnormalised=True)
    near, far = BC.random_bounds(B, P, 7)
    assert ((far - near) < 0.03 * (RC.RAY_END - RC.RAY_START)).sum() >= B * P // 4
    with torch.no_grad(), BC.per_ray_depths(near, far):
        px, dist, ref = RC.oracle_run(case)
    o, d = case.origins.numpy(), case.dirs.numpy()
    z = BC.bounded_depths(case.rng["u_strat"].numpy(), S, near, far)
    half_step = (far - near) / (2 * (S - 1)) + 1e-6              # the jitter reaches half a step beyond the interval
    assert np.array_equal(ref["coarse_z"].numpy(), z) and (z.min(-1) >= near - half_step).all() and (z.max(-1) <= far + half_step).all()
    on_device(case, dev)
    rng = dict(case.rng, fine_z=ref["fine_z"])
    for prec in ("fp32", "fp16x3"):
        case.gen.siren.precision = prec
        gpx, gdist, aux, _ = render(case, dev, rng, near, far)
        aux = {k: v.cpu().numpy() for k, v in aux.items()}
        assert np.array_equal(aux["coarse_z"], z)
        assert np.array_equal(aux["coarse_points"], RC.numpy_points(o, d, z))
        assert np.array_equal(aux["fine_points"], ref["fine_points"].numpy())
        e_c, e_f = rgb_sigma_err(aux["coarse_rgb_sigma"], ref["coarse_rgb_sigma"]), rgb_sigma_err(aux["fine_rgb_sigma"], ref["fine_rgb_sigma"])
        e_p, e_d = scaled_err(gpx.cpu().numpy(), px.numpy()), scaled_err(gdist.cpu().numpy(), dist.numpy())
        print(f"{variant} [{prec}]: rgb/sigma coarse {e_c:.2e} fine {e_f:.2e} pixels {e_p:.2e} dist {e_d:.2e}")
        assert e_c < TOL and e_f < TOL and e_p < TOL and e_d < TOL, (prec, e_c, e_f, e_p, e_d)
    # Philox draws: stream 0 at element (b P + p) S + s, as in the scalar kernel
    from oracle import philox
    seed, offset = 0x1234567890ABCDEF, 77
    _, _, aux, _ = render(case, dev, {"philox": (seed, offset)}, near, far)
    z = BC.bounded_depths(philox.uniform(seed, offset, 0, B * P * S).reshape(B, P, S), S, near, far)
    assert np.array_equal(aux["coarse_z"].cpu().numpy(), z) and np.array_equal(aux["coarse_points"].cpu().numpy(), RC.numpy_points(o, d, z))


# ---------------------------------------------------------------------------------------------------------------------
# 3. backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def backward_reference():
    """The bounded case of the backward tests and the oracle's gradients on it (fp32 and float64), computed once."""
    B, P, S = 2, 19, 12
    case = RC.make_case("SHORTSIREN_FG", 64, B, P, S, V=8, seed=29, unnormalised=True)
    near, far = BC.random_bounds(B, P, 11)
    wv = upstream(B, P)
    with BC.per_ray_depths(near, far):
        with torch.no_grad():
            forced = RC.oracle_run(case)[2]["fine_z"]
        want = RC.oracle_run(case, torch.float32, forced, wv)[3]
        exact = RC.oracle_run(case, torch.float64, forced, wv)[3]
    return case, near, far, wv, forced, want, exact


@pytest.mark.parametrize("bprec", ["fp32", "fp16"])
def test_backward_of_a_bounded_render_against_oracle_autograd(dev, backward_reference, bprec):
    """Gradients w.r.t. every parameter, the volume, the global feature, origins and dirs against float64 autograd through the oracle, which
    takes its depths from the per-ray bounds -- the tolerance rule of tests/test_gpu_render_rays.py::test_backward_against_oracle_autograd:
    fp32 scaled error < max(2e-3, 2.5 x floor); fp16 (precision fp16x3) relative L2 < max(3e-3, 2.5 x the oracle's own) and scaled error
    < max(5e-2, 2.5 x floor), nothing clamped.  near / far that require grad receive none and raise nothing."""
    from cnerf_amd import ops
    case, near, far, wv, forced, want, exact = backward_reference
    on_device(case, dev)
    net = case.gen.siren
    net.precision = "fp32" if bprec == "fp32" else "fp16x3"
    net.backward_precision = bprec
    net.zero_grad()
    t_near, t_far = torch.from_numpy(near).to(dev).requires_grad_(True), torch.from_numpy(far).to(dev).requires_grad_(True)
    px, dist, aux, leaves = render(case, dev, dict(case.rng, fine_z=forced), t_near, t_far, requires_grad=True)
    assert np.array_equal(aux["coarse_z"].cpu().numpy(), BC.bounded_depths(case.rng["u_strat"].numpy(), case.S, near, far))
    ((px * wv[0].to(dev)).sum() + (dist * wv[1].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    assert t_near.grad is None and t_far.grad is None
    if bprec == "fp16":
        assert int(ops.LAST_SATURATED.item()) == 0, "fp16 gradients were clamped"
    got = {k: p.grad for k, p in net.named_parameters()}
    got.update(volume0=leaves["vols"][0].grad, global_feature=leaves["glob"].grad, origins=leaves["origins"].grad, dirs=leaves["dirs"].grad)
    got = {k: g.double().cpu().numpy() for k, g in got.items()}
    assert set(got) == set(want), set(got) ^ set(want)
    for k, w in want.items():
        floor = scaled_err(w, exact[k])
        e, l2 = scaled_err(got[k], w), rel_l2(got[k], w)
        print(f"bounded [{bprec}] {k}: scaled_err {e:.2e} (floor {floor:.2e}) rel L2 {l2:.2e}")
        if bprec == "fp32":
            assert e < max(2e-3, 2.5 * floor), (bprec, k, e, floor)
        else:
            assert l2 < max(3e-3, 2.5 * rel_l2(w, exact[k])) and e < max(5e-2, 2.5 * floor), (bprec, k, e, l2, floor)
    assert np.abs(got["origins"]).max() > 0 and np.abs(got["dirs"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------------------------------------------------
def test_build_occupancy_ray_bounds_render(dev):
    """gen.build_occupancy -> gen.ray_bounds -> gen.render_rays(..., occupancy=grid, ray_near=, ray_far=) on V = 8, G = 8, P = 64, S = 16
    (relu, no noise, white background).  The rays start within 0.2 of the centre with |dir| = 0.35, so every sample is inside the cube;
    the threshold is the 97 % quantile of the corner densities, so that some rays cross set cells and some do not.  The first and the
    last jitter draw of every ray are 0.5: the coarse samples then lie in [ray_start, ray_end], the span the bounds speak about."""
    from cnerf_amd import ops
    G, P, S, LO, SIDE = 8, 64, 16, -1.0, 2.0
    case = RC.make_case("SHORTSIREN_FG", 64, 2, P, S, V=8, seed=13, clamp="relu", noise=0.0)
    g = torch.Generator().manual_seed(2)
    case.origins = (torch.rand(2, P, 3, generator=g) * 0.4 - 0.2).contiguous()
    d = torch.randn(2, P, 3, generator=g)
    case.dirs = (d / d.norm(dim=-1, keepdim=True) * 0.35).contiguous()
    case.rng["u_strat"][..., 0] = 0.5
    case.rng["u_strat"][..., -1] = 0.5
    on_device(case, dev)
    gen = case.gen
    z = (case.vols[0].to(dev), case.glob.to(dev))
    with torch.no_grad():
        ax = torch.tensor(LO, device=dev) + torch.arange(G + 1, device=dev, dtype=torch.float32) * (torch.tensor(SIDE, device=dev) / G)
        corners = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, -1, 3).expand(2, -1, -1).contiguous()
        threshold = float(torch.quantile(gen.siren(corners, z)[..., 3].reshape(-1), 0.97))
        grid = gen.build_occupancy(z, (LO,) * 3, SIDE, resolution=G, threshold=threshold, dilate=0)
        near, far, hit = gen.ray_bounds(grid, case.origins.to(dev), case.dirs.to(dev), RC.RAY_START, RC.RAY_END)
    words = grid.bits.cpu().numpy().view(np.uint32)
    cells = np.stack([OC.bit_at(words[b], np.arange(G ** 3)) for b in range(2)])
    hit_n, near_n, far_n = hit.cpu().numpy().astype(bool), near.cpu().numpy(), far.cpu().numpy()
    print(f"{cells.mean() * 100:.0f} % of the cells set; {hit_n.sum()} of {hit_n.size} rays hit")
    assert 0 < hit_n.sum() < hit_n.size, "the scene must have rays of both kinds"
    # ray_bounds is the ops call with pad = half a cell edge, and obeys the contract
    o_near, o_far, o_hit = ops.occupancy_ray_bounds(grid, case.origins.to(dev), case.dirs.to(dev), RC.RAY_START, RC.RAY_END, 0.5 * SIDE / G)
    assert torch.equal(o_near, near) and torch.equal(o_far, far) and torch.equal(o_hit, hit)
    pad = np.float32(0.5 * SIDE / G)
    near0, far0, hit0 = (t.cpu().numpy() for t in ops.occupancy_ray_bounds(grid, case.origins.to(dev), case.dirs.to(dev), RC.RAY_START, RC.RAY_END, 0.0))
    for b in range(2):
        o_b, d_b = case.origins[b].numpy(), case.dirs[b].numpy()
        inner, outer = BC.sandwich(o_b, d_b, cells[b], [LO] * 3, SIDE, G, RC.RAY_START, RC.RAY_END, BC.delta_of(o_b, [LO] * 3, SIDE))
        assert not BC.sandwich_violations(near0[b], far0[b], hit0[b], inner, outer, RC.RAY_START, RC.RAY_END)
    h0 = hit0.astype(bool)
    assert hit_n[h0].all()
    assert np.array_equal(near_n[h0], np.maximum(np.float32(RC.RAY_START), near0[h0] - pad))
    assert np.array_equal(far_n[h0], np.minimum(np.float32(RC.RAY_END), far0[h0] + pad))
    assert (near_n[~hit_n] == np.float32(RC.RAY_START)).all() and (far_n[~hit_n] == np.float32(RC.RAY_END)).all()
    assert (near_n[hit_n] < far_n[hit_n]).all() and ((far_n - near_n)[hit_n] < 0.9 * (RC.RAY_END - RC.RAY_START)).any()
    # the renders: unbounded masked, bounded unmasked (for the field's values and the fine depths to force), bounded masked
    rng0 = dict(case.rng)
    _, _, plain0, _ = render(case, dev, rng0)
    _, _, masked0, _ = render(case, dev, dict(rng0, fine_z=plain0["fine_z"].cpu()), occupancy=grid)
    _, _, plain, _ = render(case, dev, rng0, near, far)
    rng = dict(rng0, fine_z=plain["fine_z"].cpu())
    _, _, plain, _ = render(case, dev, rng, near, far)
    px, dist, masked, _ = render(case, dev, rng, near, far, occupancy=grid)
    N = lambda a: {k: v.cpu().numpy() for k, v in a.items()}
    plain, masked, masked0 = N(plain), N(masked), N(masked0)
    px, dist = px.cpu().numpy(), dist.cpu().numpy()
    # skipped samples hold the fill, live ones the unmasked values, bit for bit; the counts are NumPy's
    for name in ("coarse", "fine"):
        check_pass(name, masked, plain, words, G)
    assert OC.inside(masked["coarse_points"], [LO] * 3, SIDE, G).all()
    assert np.array_equal(masked["coarse_z"], BC.bounded_depths(case.rng["u_strat"].numpy(), S, near_n, far_n))
    # a ray without a set cell on its span renders the background exactly
    assert (px[~hit_n] == 1.0).all() and (dist[~hit_n] == 0.0).all()
    assert not (px[hit_n] == 1.0).all()
    # the bounded call spends its coarse samples where the cells are: at least the live samples of the unbounded masked call on the hit rays
    live0 = ~np.isneginf(masked0["coarse_rgb_sigma"][..., 3])
    on_hit = (live0 & hit_n[..., None]).sum((1, 2))
    print(f"live coarse samples: bounded {masked['live_coarse'].tolist()}, unbounded on the hit rays {on_hit.tolist()} of {live0.sum((1, 2)).tolist()}")
    assert (masked["live_coarse"] >= on_hit).all() and masked["live_coarse"].sum() > on_hit.sum()
    # and the image is the oracle's merge + composite on the masked values (skipped samples = OC.FILL) and the bounded depths
    want_px, want_dist = oracle_image(case, masked, rng)
    e_p, e_d = scaled_err(px, want_px), scaled_err(dist, want_dist)
    print(f"pixels {e_p:.2e} dist {e_d:.2e} vs float64 merge + composite")
    assert np.isfinite(px).all() and e_p < COMPOSITE_TOL and e_d < COMPOSITE_TOL, (e_p, e_d)
    skipped = np.isneginf(masked["coarse_rgb_sigma"][..., 3])
    assert OC.same_bits(masked["coarse_rgb_sigma"][skipped], np.broadcast_to(OC.FILL, (int(skipped.sum()), 4)))
