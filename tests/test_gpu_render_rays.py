"""Ray batches on the GPU: ImplicitGenerator3d.render_rays / ops.RenderRaysFunction / cnerf_render_rays_forward and _backward against
the ray oracle of tests/render_rays_common.py (the stages of oracle/render_oracle.py on caller-given rays), against the grid render,
and through ctypes alone.

Shapes: B = 2; P in {1, 37, 100} rays per image, so that P * S is no multiple of 32 and the last 32-point tile of an image is ragged;
S in {10, 33} (2 S = 66 merged samples cross a 64-lane chunk) and one case P = 3, S = 128 (2 S = 256: the LDS bound of the merge); H in
{64, 256}, V = 8; origins on spheres of radius 1 - 1.5 aimed near the centre, directions of length 0.7 - 1.3 in the P = 37 cases.
Gates: rgb / sigma 1e-4 (fp32, fp16x3), 1e-1 (fp16: the property tolerance of test_gpu_parity.py::test_single_pass_fp16); image 1e-4
with the oracle's fine depths forced; gradients as tests/test_gpu_field_query_grad.py: the fp32 oracle is the target, its float64
run the floor."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_rays_common as RC
from conftest import scaled_err
from oracle import philox, render_oracle as O
from oracle.checks import flips_outside_band, merge_order_matches, rgb_sigma_err

pytestmark = pytest.mark.gpu

TOL = 1e-4
SHAPES = [dict(P=1, S=10, H=64), dict(P=37, S=33, H=256), dict(P=100, S=10, H=64), dict(P=3, S=128, H=64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def on_device(case, dev):
    case.gen.to(dev)
    case.gen.set_device(dev)
    case.gen.eval()


def render(case, dev, rng, requires_grad=False):
    """gen.render_rays on the case's rays with the draws `rng` -> (pixels, dist, aux, leaves)."""
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(requires_grad)
    vols, glob, o, d = [leaf(v) for v in case.vols], leaf(case.glob), leaf(case.origins), leaf(case.dirs)
    aux = {}
    with torch.set_grad_enabled(requires_grad):
        px, dist = case.gen.render_rays(RC.generator_z(case, vols, glob), o, d, RC.RAY_START, RC.RAY_END, case.S, case.hierarchical,
                                        clamp_mode=case.clamp, nerf_noise=case.noise, white_back=case.white_back, last_back=case.last_back,
                                        _rng={k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in rng.items()}, _aux=aux)
    return px, dist, aux, dict(vols=vols, glob=glob, origins=o, dirs=d)


# ---------------------------------------------------------------------------------------------------------------------
# 1. geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_geometry_is_the_stated_arithmetic(dev, shape):
    """coarse_z, coarse_points, fine_points bit-equal to the NumPy float32 statement of include/cnerf.h: z = zl[s] + (u - 0.5)(zl[1] - zl[0]),
    p = o + d z with the product rounded before the sum -- with injected draws and forced fine depths, and with Philox draws (stream 0 at
    element (b P + p) S + s; the fine positions then at the depths the device resampled)."""
    P, S, H = shape["P"], shape["S"], shape["H"]
    case = RC.make_case("SHORTSIREN_FG", H, 2, P, S, seed=P + S, unnormalised=P == 37)
    on_device(case, dev)
    o, d = case.origins.numpy(), case.dirs.numpy()
    forced = RC.RAY_START + (RC.RAY_END - RC.RAY_START) * torch.rand(2, P, S, generator=torch.Generator().manual_seed(3))
    _, _, aux, _ = render(case, dev, dict(case.rng, fine_z=forced))
    z, pts = RC.numpy_geometry(o, d, case.rng["u_strat"].numpy(), S, RC.RAY_START, RC.RAY_END)
    assert np.array_equal(aux["coarse_z"].cpu().numpy(), z)
    assert np.array_equal(aux["coarse_points"].cpu().numpy(), pts)
    assert np.array_equal(aux["fine_points"].cpu().numpy(), RC.numpy_points(o, d, forced.numpy()))
    seed, offset = 0x1234567890ABCDEF, 77
    _, _, aux, _ = render(case, dev, {"philox": (seed, offset)})
    u = philox.uniform(seed, offset, 0, 2 * P * S).reshape(2, P, S)
    z, pts = RC.numpy_geometry(o, d, u, S, RC.RAY_START, RC.RAY_END)
    assert np.array_equal(aux["coarse_z"].cpu().numpy(), z)
    assert np.array_equal(aux["coarse_points"].cpu().numpy(), pts)
    fz = aux["fine_z"].cpu().numpy()
    assert np.isfinite(fz).all() and np.array_equal(aux["fine_points"].cpu().numpy(), RC.numpy_points(o, d, fz))


# ---------------------------------------------------------------------------------------------------------------------
# 2. forward against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "SHORTSIREN", "SHORTSIREN_FRes", "TALLSIREN"])
def test_forward_against_the_oracle(dev, variant, shape):
    P, S, H = shape["P"], shape["S"], shape["H"]
    B = 2
    # seeds: 10 + P + S, except where that case's own cdf conditioning (RC.cdf_conditioning: 2e-7 .. 6e-7 at 256 merged samples, and it moves
    # by a fifth between hosts) came within a fifth of the 5e-7 asserted below -- there the first of seed + 100 k that gives < 3e-7
    seed = {("SHORTSIREN", 128): 541, ("SHORTSIREN_FRes", 128): 341, ("TALLSIREN", 128): 341}.get((variant, S), 10 + P + S)
    case = RC.make_case(variant, H, B, P, S, seed=seed, unnormalised=P == 37, clamp="relu" if (variant, P) == ("SHORTSIREN_FG", 100) else "softplus")
    with torch.no_grad():
        px, dist, ref = RC.oracle_run(case)
        _, _, exact = RC.oracle_run(case, torch.float64)
    u = case.rng["u_fine"].numpy()
    # the resampling check below needs draws away from the cdf entries: at most 1 % inside the 2e-6 band, and the oracle's own fp32 bin
    # indices equal to its float64 run's outside it -- checked here on the CPU (seeds are chosen for it)
    assert RC.in_band_share(ref["cdf"].numpy(), u) <= 0.01
    assert RC.cdf_conditioning(case, ref) < 5e-7          # half the 1e-6 gate on the cdf below is left to the device
    assert flips_outside_band(ref["cdf"].numpy(), u, ref["inds"].numpy(), exact["inds"].numpy(), 2e-6)[0] == 0
    on_device(case, dev)
    rng = dict(case.rng, fine_z=ref["fine_z"])
    for prec in ("fp32", "fp16x3", "fp16"):
        case.gen.siren.precision = prec
        gpx, gdist, aux, _ = render(case, dev, rng)
        aux = {k: v.cpu().numpy() for k, v in aux.items()}
        assert np.array_equal(aux["coarse_points"], ref["coarse_points"].numpy()) and np.array_equal(aux["fine_points"], ref["fine_points"].numpy())
        e_c, e_f = rgb_sigma_err(aux["coarse_rgb_sigma"], ref["coarse_rgb_sigma"]), rgb_sigma_err(aux["fine_rgb_sigma"], ref["fine_rgb_sigma"])
        print(f"{variant} {shape} [{prec}]: rgb/sigma scaled_err coarse {e_c:.2e} fine {e_f:.2e}")
        if prec == "fp16":
            assert e_c < 1e-1 and e_f < 1e-1, (prec, e_c, e_f)
            continue
        assert e_c < TOL and e_f < TOL, (prec, e_c, e_f)
        e_p, e_d = scaled_err(gpx.cpu().numpy(), px.numpy()), scaled_err(gdist.cpu().numpy(), dist.numpy())
        print(f"    pixels {e_p:.2e} dist {e_d:.2e}")
        assert e_p < TOL and e_d < TOL, (prec, e_p, e_d)
        # wiring of the resampling: the oracle's stage on the DEVICE's coarse rgb_sigma
        dz, drs = torch.from_numpy(aux["coarse_z"]), torch.from_numpy(aux["coarse_rgb_sigma"])
        _, _, w = O.composite(drs, dz, case.rng["eps_coarse"], case.noise, case.clamp)
        _, inds, cdf = O.importance_depths(dz, w, case.rng["u_fine"])
        assert scaled_err(aux["coarse_weights"], w.numpy()) < 1e-5
        assert scaled_err(aux["cdf"], cdf.numpy()) < 1e-6
        hard, frac = flips_outside_band(cdf.numpy(), u, aux["inds"], inds.numpy().astype(np.int32), 2e-6)
        assert hard == 0 and frac < 1e-3, (hard, frac)
        assert merge_order_matches(aux["sort_idx"], ref["sort_idx"].numpy(), ref["fine_z"].numpy(), ref["coarse_z"].numpy())
        assert scaled_err(aux["final_weights"], ref["final_weights"].numpy()) < 5e-4


# ---------------------------------------------------------------------------------------------------------------------
# 3. backward against float64 autograd through the oracle
# ---------------------------------------------------------------------------------------------------------------------
def upstream(B, P, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, P, 3, generator=g), torch.randn(B, P, generator=g)


_oracle_cache = {}


def oracle_gradients(key, case, forced, wv):
    """(fp32 gradients, float64 gradients) of the case, computed once per key and shared (read only)."""
    if key not in _oracle_cache:
        want = RC.oracle_run(case, torch.float32, forced, wv)[3]
        exact = RC.oracle_run(case, torch.float64, forced, wv)[3]
        _oracle_cache[key] = (want, exact)
    return _oracle_cache[key]


def gpu_gradients(case, dev, rng, wv, backward_precision):
    from cnerf_amd import ops
    net = case.gen.siren
    net.precision = "fp32" if backward_precision == "fp32" else "fp16x3"
    net.backward_precision = backward_precision
    net.zero_grad()
    px, dist, _, leaves = render(case, dev, rng, requires_grad=True)
    ((px * wv[0].to(dev)).sum() + (dist * wv[1].to(dev)).sum()).backward()
    torch.cuda.synchronize()
    if backward_precision == "fp16":
        assert int(ops.LAST_SATURATED.item()) == 0, "fp16 gradients were clamped"
    got = {k: p.grad for k, p in net.named_parameters()}
    got.update({f"volume{i}": v.grad for i, v in enumerate(leaves["vols"])})
    if leaves["glob"] is not None:
        got["global_feature"] = leaves["glob"].grad
    got.update(origins=leaves["origins"].grad, dirs=leaves["dirs"].grad)
    return {k: g.double().cpu().numpy() for k, g in got.items()}


BACKWARD_CASES = {
    "fg_forced": dict(variant="SHORTSIREN_FG", H=64, P=37, S=33, precisions=("fp32", "fp16"), unnormalised=True, outside_ray=True),
    "fg_one_ray": dict(variant="SHORTSIREN_FG", H=256, P=1, S=10, precisions=("fp32",)),
    "fg_256_samples": dict(variant="SHORTSIREN_FG", H=64, P=3, S=128, precisions=("fp32", "fp16")),
    "fg_not_hierarchical": dict(variant="SHORTSIREN_FG", H=64, P=100, S=10, precisions=("fp32",), hierarchical=False, outside_ray=True),
    "global_latent": dict(variant="SHORTSIREN", H=64, P=100, S=10, precisions=("fp32",)),
    "per_point_film": dict(variant="TALLSIREN", H=64, P=37, S=10, precisions=("fp32",), unnormalised=True),
    "pyramid": dict(variant="SHORTSIREN_FG_Pyrmd", H=256, P=37, S=33, precisions=("fp16",), outside_ray=True),
}


def backward_case(name):
    c = dict(BACKWARD_CASES[name])
    precisions = c.pop("precisions")
    case = RC.make_case(c.pop("variant"), c.pop("H"), 2, c.pop("P"), c.pop("S"), seed=len(name), **c)
    wv = upstream(case.B, case.P)
    forced = None
    if case.hierarchical:       # teacher forcing: the fp32 oracle's resampled depths, on every side
        with torch.no_grad():
            forced = RC.oracle_run(case)[2]["fine_z"]
    want, exact = oracle_gradients(name, case, forced, wv)
    rng = dict(case.rng, fine_z=forced) if forced is not None else dict(case.rng)
    return case, wv, rng, want, exact, precisions


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_against_oracle_autograd(dev, name):
    """Loss sum(w_p * pixels) + sum(v * dist) with random w_p, v: every parameter, volume level, the global feature, origins and dirs.
    fp32 backward: scaled error < max(2e-3, 2.5 x floor); fp16: relative L2 < max(3e-3, 2.5 x the oracle's own) and scaled error
    < max(5e-2, 2.5 x floor), nothing clamped."""
    case, wv, rng, want, exact, precisions = backward_case(name)
    on_device(case, dev)
    for bprec in precisions:
        got = gpu_gradients(case, dev, rng, wv, bprec)
        assert set(got) == set(want), set(got) ^ set(want)
        for k, w in want.items():
            floor = scaled_err(w, exact[k])
            e, l2 = scaled_err(got[k], w), rel_l2(got[k], w)
            print(f"{name} [{bprec}] {k}: scaled_err {e:.2e} (floor {floor:.2e}) rel L2 {l2:.2e}")
            if bprec == "fp32":
                assert e < max(2e-3, 2.5 * floor), (name, bprec, k, e, floor)
            else:
                assert l2 < max(3e-3, 2.5 * rel_l2(w, exact[k])) and e < max(5e-2, 2.5 * floor), (name, bprec, k, e, l2, floor)
        assert np.abs(got["origins"]).max() > 0 and np.abs(got["dirs"]).max() > 0
        if BACKWARD_CASES[name].get("outside_ray"):
            # a feature-volume family without an xyz input: every sample of ray (0, 0) lies beyond the lookup's clamp on every axis
            assert (RC.ray_points(case.origins, case.dirs, RC.ray_depths(case.rng["u_strat"], case.S, RC.RAY_START, RC.RAY_END))[0, 0] > 0.6).all()
            assert np.all(got["origins"][0, 0] == 0.0) and np.all(got["dirs"][0, 0] == 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. against the grid render
# ---------------------------------------------------------------------------------------------------------------------
def test_against_the_grid_render(golden, dev):
    """short_fg_smooth with its u_strat and forced fine depths, the grid's own world rays: render_rays agrees with forward within
    max(1e-4, 2.5 x the oracle-level floor of tests/test_render_rays_cpu.py); a non-square crop of rays renders bit for bit what the
    same rays render inside the full batch; pinhole_rays gives the grid's rays to 1e-6."""
    from test_gpu_parity import G, make_generator, make_z
    from test_render_rays_cpu import PIXEL_FLOOR
    from cnerf_amd.generators.volumetric_rendering import pinhole_rays
    g = golden("short_fg_smooth")
    m = g.meta
    B, R, S = m["B"], m["R"], m["S"]
    P = R * R
    gen = make_generator(g, dev)
    z, _, _ = make_z(g, dev)
    cam = torch.from_numpy(g["cam2worlds"])
    z_lin, offset, _ = O.stratified_depths(B, R, S, m["ray_start"], m["ray_end"], torch.from_numpy(g["u_strat"]))
    _, dirs_w, org = O.coarse_world_points(cam, O.camera_ray_dirs(R, m["fov"]), z_lin, offset)
    origins = org.reshape(B, 1, 3).expand(B, P, 3).contiguous().to(dev)
    dirs = dirs_w.to(dev)
    rng = {k: G(g[k], dev) for k in ("u_strat", "u_fine", "fine_z")}
    kw = dict(clamp_mode=m["clamp"], nerf_noise=m["noise"], white_back=m["white_back"], last_back=m["last_back"])
    with torch.no_grad():
        px_grid, depth = gen(z, cam.to(dev), R, m["fov"], m["ray_start"], m["ray_end"], S, True, _rng=dict(rng), **kw)
        aux = {}
        px, dist = gen.render_rays(z, origins, dirs, m["ray_start"], m["ray_end"], S, True, _rng=dict(rng), _aux=aux, **kw)
    assert np.array_equal(aux["coarse_z"].cpu().numpy(), g["coarse_z"]) and np.array_equal(aux["fine_points"].cpu().numpy(), g["fine_points"])
    e = scaled_err(px.cpu().numpy(), px_grid.reshape(B, 3, P).permute(0, 2, 1).cpu().numpy())
    print(f"render_rays vs forward on the grid's rays: pixels scaled_err {e:.2e}")
    assert e < max(1e-4, 2.5 * PIXEL_FLOOR["short_fg_smooth"]), e
    dz = O.camera_ray_dirs(R, m["fov"])[:, 2].reshape(1, P).to(dev)
    assert scaled_err((dist * dz).cpu().numpy(), depth.reshape(B, P).cpu().numpy()) < max(1e-4, 2.5 * PIXEL_FLOOR["short_fg_smooth"])
    # a crop, rows 3-9 and columns 5-16 (6 x 11: not square)
    rows, cols = torch.arange(3, 9), torch.arange(5, 16)
    idx = (rows[:, None] * R + cols[None, :]).reshape(-1).to(dev)
    crop = lambda t: t[:, idx].contiguous()
    with torch.no_grad():
        px_c, dist_c = gen.render_rays(z, crop(origins), crop(dirs), m["ray_start"], m["ray_end"], S, True, _rng={k: crop(v) for k, v in rng.items()}, **kw)
    assert px_c.shape == (B, 66, 3) and torch.equal(px_c, px[:, idx]) and torch.equal(dist_c, dist[:, idx])
    # pinhole_rays: the grid's rays to rounding, crops by rows / columns
    po, pd = pinhole_rays(cam.to(dev), R, m["fov"])
    assert torch.equal(po, origins) and (pd - dirs).abs().max().item() < 1e-6
    co, cd = pinhole_rays(cam.to(dev), R, m["fov"], rows=rows, cols=cols)
    assert torch.equal(co, po[:, idx]) and torch.equal(cd, pd[:, idx])


# ---------------------------------------------------------------------------------------------------------------------
# 5. chunking and determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bprec", ["fp32", "fp16"])
def test_gradients_do_not_depend_on_the_chunking_and_repeat_bit_for_bit(dev, monkeypatch, bprec):
    """ops.query_chunk forced to 64 points per chunk (370 points per image: five full chunks and a 50-point tail) against one chunk per
    image -- the gates of test_gpu_field_query_grad.py::test_query_gradients_do_not_depend_on_the_chunking: sums in another order (fp32
    1e-4 scaled; fp16 2e-3 relative L2: per-chunk gradient scales) -- and grad_origins / grad_dirs of two identical runs bit-equal."""
    from cnerf_amd import ops
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 10, seed=31, unnormalised=True)
    wv = upstream(case.B, case.P)
    with torch.no_grad():
        forced = RC.oracle_run(case)[2]["fine_z"]
    on_device(case, dev)
    rng = dict(case.rng, fine_z=forced)
    real = ops.query_chunk
    seen = []

    def small(n, bytes_of, d):
        seen.append(n)
        return 64, bytes_of(64)
    res = []
    for chunk in (real, real, small):
        monkeypatch.setattr(ops, "query_chunk", chunk)
        res.append(gpu_gradients(case, dev, rng, wv, bprec))
    monkeypatch.setattr(ops, "query_chunk", real)
    assert seen == [case.P * case.S], "the chunk-size patch was not applied"
    assert np.array_equal(res[0]["origins"], res[1]["origins"]) and np.array_equal(res[0]["dirs"], res[1]["dirs"])
    for k in res[0]:
        if bprec == "fp32":
            assert scaled_err(res[2][k], res[0][k]) < 1e-4, (k, scaled_err(res[2][k], res[0][k]))
        else:
            assert rel_l2(res[2][k], res[0][k]) < 2e-3, (k, rel_l2(res[2][k], res[0][k]))


# ---------------------------------------------------------------------------------------------------------------------
# the public interface
# ---------------------------------------------------------------------------------------------------------------------
def test_generator_interface(dev):
    """rng_mode "torch" draws what draw_rng(B, P, S, ...) draws, in its order; "philox" renders without tensors; under no_grad there is
    no autograd node and the image equals the differentiable one's; a training-mode network with drop_out raises NotImplementedError."""
    from cnerf_amd.generators import ImplicitGenerator3d
    from cnerf_amd.generators.generators import draw_rng
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 10, seed=41)
    on_device(case, dev)
    gen = case.gen
    z = (case.vols[0].to(dev), case.glob.to(dev))
    o, d = case.origins.to(dev), case.dirs.to(dev)
    args = (RC.RAY_START, RC.RAY_END, case.S, True)
    kw = dict(clamp_mode="softplus", nerf_noise=0.3, white_back=True)
    with torch.no_grad():
        torch.manual_seed(5)
        a = gen.render_rays(z, o, d, *args, **kw)
        torch.manual_seed(5)
        b = gen.render_rays(z, o, d, *args, _rng=draw_rng(2, 37, case.S, True, 0.3, dev), **kw)
        assert a[0].grad_fn is None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        gen.rng_mode = "philox"
        p = gen.render_rays(z, o, d, *args, **kw)
        assert p[0].shape == (2, 37, 3) and p[1].shape == (2, 37) and torch.isfinite(p[0]).all() and not torch.equal(p[0], a[0])
        gen.rng_mode = "torch"
    torch.manual_seed(5)
    od = o.clone().requires_grad_(True)
    c = gen.render_rays(z, od, d, *args, **kw)
    assert c[0].grad_fn is not None and torch.equal(c[0].detach(), a[0])
    dropping = ImplicitGenerator3d("SHORTSIREN_FG", 32, 32, 4, 64, drop_out=0.2).to(dev)
    dropping.set_device(dev)
    dropping.train()
    with pytest.raises(NotImplementedError, match="forward"):
        dropping.render_rays(z, o, d, *args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 6. ctypes only
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_through_ctypes_only(dev):
    """One forward + backward through the four ray-batch entries with raw device pointers -- no cnerf_amd.ops, no autograd -- against
    the oracle numbers of test_backward_against_oracle_autograd's "fg_forced" case (fp32 gates)."""
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    case, wv, rng_t, want, exact, _ = backward_case("fg_forced")
    B, P, S, H, V = case.B, case.P, case.S, case.H, 8
    T = lambda t: t.detach().to(dev).contiguous()
    dptr = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc, what):
        assert rc == 0, f"{what}: rc {rc}: {lib.cnerf_last_error().decode()}"

    prm = {k: T(v) for k, v in case.gen.siren.state_dict().items()}
    cfg = L.Cfg()
    cfg.B, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, S, V, 32, H, 4
    for i in range(4):
        cfg.layer_kind[i] = L.LAYER_FILM
    cfg.ray_start, cfg.ray_end, cfg.voxel_length, cfg.noise_std = RC.RAY_START, RC.RAY_END, 1.2, case.noise
    cfg.flags = L.F_HIERARCHICAL | L.F_WHITE_BACK | L.F_SOFTPLUS | L.F_SIGMOID_RGB
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, V, 32
    cfg.precision = L.PREC_FP32
    fp, gp, grads = L.FieldParams(), L.FieldParamGrads(), {}
    for i in range(4):
        for slot, suffix in (("w", "weight"), ("b", "bias")):
            k = f"network.{i}.layer.{suffix}"
            grads[k] = torch.zeros_like(prm[k])
            getattr(fp, slot)[i], getattr(gp, slot)[i] = prm[k].data_ptr(), grads[k].data_ptr()
    for slot, suffix in (("w_final", "weight"), ("b_final", "bias")):
        k = f"final_layer.{suffix}"
        grads[k] = torch.zeros_like(prm[k])
        setattr(fp, slot, prm[k].data_ptr())
        setattr(gp, slot, grads[k].data_ptr())
    glob = T(case.glob)
    fo = torch.nn.functional.linear(glob, prm["mapping_network.weight"], prm["mapping_network.bias"])      # the FiLM mapping Linear stays on the host
    freq, phase = (fo[:, :4 * H] * 15 + 30).contiguous(), fo[:, 4 * H:].contiguous()
    fvol = T(case.vols[0])
    fcl = torch.empty((B, V, V, V, 32), device=dev)
    ok(lib.cnerf_fvol_channel_last(B, 32, V, dptr(fvol), dptr(fcl), stream), "channel_last")
    vols = L.Volumes()
    vols.level[0] = fcl.data_ptr()
    nb = C.c_size_t()
    ok(lib.cnerf_workspace_bytes(C.byref(cfg), C.byref(nb), None, None), "workspace_bytes")
    packed = torch.empty(nb.value // 4, device=dev)
    ok(lib.cnerf_pack_field(C.byref(cfg), C.byref(fp), dptr(packed), stream), "pack_field")
    ok(lib.cnerf_render_rays_workspace_bytes(C.byref(cfg), P, C.byref(nb)), "render_rays_workspace_bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    origins, dirs = T(case.origins), T(case.dirs)
    rays = L.Rays()
    rays.origins, rays.dirs = origins.data_ptr(), dirs.data_ptr()
    draws = {k: T(v) for k, v in rng_t.items()}
    rng = L.Rng()
    for k, t in draws.items():
        setattr(rng, k, t.data_ptr())
    aux = L.Aux()
    sv = dict(coarse_rgb_sigma=torch.empty((B, P, S, 4), device=dev), coarse_z=torch.empty((B, P, S), device=dev),
              fine_rgb_sigma=torch.empty((B, P, S, 4), device=dev))
    for k, t in sv.items():
        setattr(aux, k, t.data_ptr())
    pixels, dist = torch.empty((B, P, 3), device=dev), torch.empty((B, P), device=dev)
    ok(lib.cnerf_render_rays_forward(C.byref(cfg), C.byref(rays), P, C.byref(vols), dptr(packed), dptr(freq), dptr(phase), C.byref(rng), dptr(pixels),
                                     dptr(dist), C.byref(aux), dptr(ws), stream), "render_rays_forward")
    with torch.no_grad():
        px, ds, _ = RC.oracle_run(case, forced_fine_z=rng_t["fine_z"])
    assert scaled_err(pixels.cpu().numpy(), px.numpy()) < TOL and scaled_err(dist.cpu().numpy(), ds.numpy()) < TOL

    ok(lib.cnerf_backward_bytes(C.byref(cfg), C.byref(nb)), "backward_bytes")
    packed_t = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    ok(lib.cnerf_pack_field_transposed(C.byref(cfg), C.byref(fp), dptr(packed_t), stream), "pack_field_transposed")
    ppc = 500                      # 1221 points per image: two full chunks and a 221-point tail
    ok(lib.cnerf_render_rays_backward_workspace_bytes(C.byref(cfg), L.PREC_FP32, P, ppc, C.byref(nb)), "render_rays_backward_workspace_bytes")
    bws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    saved = L.Saved()
    for k, t in sv.items():
        setattr(saved, k, t.data_ptr())
    saved.fine_z = draws["fine_z"].data_ptr()          # the depths the fine pass used
    g_freq, g_phase, g_vol = torch.zeros_like(freq), torch.zeros_like(phase), torch.zeros_like(fcl)
    gvols = L.Volumes()
    gvols.level[0] = g_vol.data_ptr()
    g_org, g_dir = torch.zeros_like(origins), torch.zeros_like(dirs)
    grad_pixels, grad_dist = T(wv[0]), T(wv[1])
    ok(lib.cnerf_render_rays_backward(C.byref(cfg), L.PREC_FP32, ppc, C.byref(rays), P, C.byref(vols), C.byref(fp), dptr(packed), dptr(packed_t),
                                      dptr(freq), dptr(phase), C.byref(rng), C.byref(saved), dptr(grad_pixels), dptr(grad_dist), C.byref(gp), dptr(g_freq),
                                      dptr(g_phase), C.byref(gvols), dptr(g_org), dptr(g_dir), None, dptr(bws), stream), "render_rays_backward")
    torch.cuda.synchronize()
    gv_cf = torch.empty_like(fvol)
    ok(lib.cnerf_fvol_channel_first(B, 32, V, dptr(g_vol), dptr(gv_cf), stream), "channel_first")
    d_fo = torch.cat([15.0 * g_freq, g_phase], -1)          # the host finishes the mapping Linear
    got = dict(grads, volume0=gv_cf, origins=g_org, dirs=g_dir, global_feature=d_fo @ prm["mapping_network.weight"])
    got["mapping_network.weight"], got["mapping_network.bias"] = d_fo.t() @ glob, d_fo.sum(0)
    assert set(got) == set(want)
    for k, w in want.items():
        e, floor = scaled_err(got[k].cpu().numpy(), w), scaled_err(w, exact[k])
        assert e < max(2e-3, 2.5 * floor), (k, e, floor)
