"""SHORTSIREN on the GPU: a FiLM field on the sample's world position, no feature volume (CNERF_F_NO_VOLUME, the no-lookup
instantiation of the fp32 field kernels), driven by one global latent through the mapping MLP.  Against the reference's own
numbers (fixtures aux_shortsiren_small / aux_shortsiren_softplus, tests/golden/make_golden_global.py) and against a float64
restatement of the network composed with the oracle's ray stages (tests/global_latent_common.py).

Gates are the project's own: rgb / sigma 1e-4 scaled (oracle.checks.rgb_sigma_err) in fp32 and fp16x3, the 1e-1 of
tests/test_gpu_parity.py::test_single_pass_fp16 in single-pass fp16; gradients as in
tests/test_gpu_field_query_grad.py::test_query_gradients_vs_oracle_autograd -- fp32 backward: scaled error < max(2e-3, 2.5 x the
fp32-vs-float64 floor of the same restatement); fp16 backward: relative L2 < max(3e-3, 2.5 x floor) and scaled error < max(5e-2,
2.5 x floor)."""
import ctypes as C

import numpy as np
import pytest
import torch

import global_latent_common as GL
from conftest import scaled_err
from oracle.checks import bin_mass, flips_outside_band, merge_order_matches, random_weight_loss, rgb_sigma_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
FIXTURES = ["aux_shortsiren_small", "aux_shortsiren_softplus"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


_cache = {}


def fx(name):
    if name not in _cache:
        _cache[name] = GL.fixture(name)
    return _cache[name]


def T(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def on_gpu(gen, dev, train=False):
    gen.to(dev)
    gen.set_device(dev)
    gen.train(train)
    return gen


def render_kwargs(m):
    return dict(clamp_mode=m["clamp"], nerf_noise=m["noise"], white_back=m["white_back"], last_back=m["last_back"])


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def set_precision(gen, bprec):
    """backward precision "fp32": everything fp32; "fp16": the fp16x3 forward and the fp16 gradient chain."""
    gen.siren.precision = "fp32" if bprec == "fp32" else "fp16x3"
    gen.siren.backward_precision = bprec


def check_grads(tag, got, want, exact, bprec):
    from cnerf_amd import ops
    assert set(got) == set(want), set(got) ^ set(want)
    if bprec == "fp16":
        assert int(ops.LAST_SATURATED.item()) == 0, "fp16 gradients were clamped"
    for k, wv in want.items():
        floor, e, l2 = scaled_err(wv, exact[k]), scaled_err(got[k], wv), rel_l2(got[k], wv)
        print(tag, bprec, k, "err", e, "rel l2", l2, "floor", floor)
        if bprec == "fp32":
            assert e < max(2e-3, 2.5 * floor), (tag, bprec, k, e, floor)
        else:
            assert l2 < max(3e-3, 2.5 * rel_l2(wv, exact[k])) and e < max(5e-2, 2.5 * floor), (tag, bprec, k, e, l2, floor)


def fixture_rng(g, dev, forced):
    rng = {k: T(g.get(k), dev) for k in ("u_strat", "eps_coarse", "u_fine", "eps_final") if g.get(k) is not None}
    if forced:
        rng["fine_z"] = T(g["fine_z"], dev)
    return rng


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,gate", [("fp32", TOL), ("fp16x3", TOL), ("fp16", 1e-1)])
@pytest.mark.parametrize("name", FIXTURES)
def test_field_forward_at_the_reference_points(dev, name, precision, gate):
    """generator.siren(points, z) at the reference's own sample positions of both passes: fp32 and fp16x3 within the 1e-4 scaled
    gate, single-pass fp16 within the bound of test_single_pass_fp16."""
    g = fx(name)
    gen = on_gpu(GL.make_generator(g), dev)
    gen.siren.precision = precision
    z = T(g["z"], dev)
    B = z.shape[0]
    for key in ("coarse", "fine"):
        with torch.no_grad():
            out = gen.siren(T(g[key + "_points"], dev).reshape(B, -1, 3), z)
        e = rgb_sigma_err(out.cpu().numpy().reshape(g[key + "_rgb_sigma"].shape), g[key + "_rgb_sigma"])
        print(name, precision, key, "rgb_sigma_err", e)
        assert e < gate, (name, precision, key, e)


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("n", [31, 32, 33])
def test_field_forward_ragged_point_counts(dev, n, H, precision):
    """31, 32 and 33 points per image (a partial tile, a full one, a full one and a single point) against the float64 restatement."""
    gen = GL.fresh_generator(H, seed=n)
    torch.manual_seed(100 + n)
    z, pts = torch.randn(2, 32), (torch.rand(2, n, 3) * 2 - 1) * 0.9
    exact = GL.field(GL.cast_params(gen.siren, torch.float64), z.double(), pts.double()).detach().numpy()
    on_gpu(gen, dev)
    gen.siren.precision = precision
    with torch.no_grad():
        out = gen.siren(pts.to(dev), z.to(dev))
    assert out.shape == (2, n, 4)
    e = rgb_sigma_err(out.cpu().numpy(), exact)
    print("ragged", n, H, precision, e)
    assert e < TOL, (n, H, e)


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("name", FIXTURES)
def test_render_against_the_reference(dev, name, precision):
    """ImplicitGenerator3d("SHORTSIREN").forward(z, cam2worlds, ...) with the reference's draws.  Geometry bit-exact; with the
    reference's fine depths forced: rgb / sigma, pixels and depth within 1e-4 and the reference's merge order; free-running: the
    resampling decisions equal the reference's outside the guard band of test_resample_stage."""
    g = fx(name)
    m = g.meta
    gen = on_gpu(GL.make_generator(g), dev)
    gen.siren.precision = precision
    z, cam = T(g["z"], dev), T(g["cam2worlds"], dev)
    out = {}
    for forced in (True, False):
        aux = {}
        with torch.no_grad():
            px, dp = gen(z, cam, m["R"], m["fov"], m["ray_start"], m["ray_end"], m["S"], True, _rng=fixture_rng(g, dev, forced), _aux=aux,
                         batch_size=7, **render_kwargs(m))
        torch.cuda.synchronize()
        out[forced] = (px.cpu().numpy(), dp.cpu().numpy(), {k: v.cpu().numpy() for k, v in aux.items()})
    px, dp, aux = out[True]
    assert np.array_equal(aux["coarse_points"], g["coarse_points"])
    assert np.array_equal(aux["coarse_z"], g["coarse_z"])
    # fine points = origin + direction * depth.  The reference forms the 36 world directions of this image size with a 3x3 BLAS
    # product whose rounding (fused chain or not) depends on the micro-kernel its host picks for that size; a last-bit change
    # of a direction component (6e-8) times a depth below 2, plus the sum's own rounding below 2 (1.2e-7): 2.4e-7, bound 5e-7
    dfp = float(np.abs(aux["fine_points"] - g["fine_points"]).max())
    print(name, "fine points max |diff|", dfp, "differing", int((aux["fine_points"] != g["fine_points"]).sum()), "of", g["fine_points"].size)
    assert dfp < 5e-7
    ec, ef = rgb_sigma_err(aux["coarse_rgb_sigma"], g["coarse_rgb_sigma"]), rgb_sigma_err(aux["fine_rgb_sigma"], g["fine_rgb_sigma"])
    ep, ed = scaled_err(px, g["pixels"]), scaled_err(dp, g["depth"])
    print(name, precision, "forced: coarse", ec, "fine", ef, "pixels", ep, "depth", ed)
    assert ec < TOL and ef < TOL
    assert merge_order_matches(aux["sort_idx"], g["sort_idx"], g["fine_z"], g["coarse_z"])
    assert ep <= TOL and ed <= TOL
    _, _, free = out[False]
    assert np.array_equal(free["coarse_points"], g["coarse_points"])
    hard, frac = flips_outside_band(g["cdf"], g["u_fine"], free["inds"], g["inds"].astype(np.int32), 2e-6)
    print(name, "free-running: flips outside the band", hard, "fraction of differing draws", frac)
    assert hard == 0


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def gpu_render_grads(gen, g_or_meta, z, cam, rng, dev, R, S, loss):
    m = g_or_meta
    gen.zero_grad()
    zd = z.to(dev).requires_grad_(True)
    px, dp = gen(zd, cam.to(dev), R, m["fov"], m["ray_start"], m["ray_end"], S, True, _rng={k: v.to(dev) for k, v in rng.items()}, **render_kwargs(m))
    loss(px, dp).backward()
    torch.cuda.synchronize()
    got = {k: p.grad.double().cpu().numpy() for k, p in gen.named_parameters()}
    got["z"] = zd.grad.double().cpu().numpy()
    return got, px.detach().cpu(), dp.detach().cpu()


def test_render_backward_against_the_reference(dev):
    """fp32 backward against the fixture's gradients (the reference's autograd under oracle.checks.random_weight_loss, its own fine
    depths forced here): every parameter, the four mapping Linears included, and z.  Floor: the float64 restatement on the same positions."""
    g = fx("aux_shortsiren_small")
    m = g.meta
    gen = GL.make_generator(g)
    z, cam = torch.from_numpy(g["z"]), torch.from_numpy(g["cam2worlds"])
    u_strat, u_fine, fz = (torch.from_numpy(g[k]) for k in ("u_strat", "u_fine", "fine_z"))
    loss = random_weight_loss(m["B"], m["R"])
    exact = {}
    p64 = GL.cast_params(gen.siren, torch.float64, True)
    z64 = z.double().requires_grad_(True)
    px, dp, _ = GL.render(p64, z64, cam, m, u_strat, u_fine, forced_fine_z=fz)
    grads = torch.autograd.grad(loss(px, dp), list(p64.values()) + [z64])
    exact = {"siren." + k: v.numpy() for k, v in zip(p64, grads[:-1])}
    exact["z"] = grads[-1].numpy()
    on_gpu(gen, dev)
    got, _, _ = gpu_render_grads(gen, m, z, cam, {"u_strat": u_strat, "u_fine": u_fine, "fine_z": fz}, dev, m["R"], m["S"], loss)
    checked = 0
    for k in got:
        want, mine, ex = (g["grad_z"] if k == "z" else g["grad/" + k]), got[k], exact[k]
        assert want.shape == mine.shape
        floor, e = scaled_err(want, ex), scaled_err(mine, want)
        print("render backward vs reference", k, "err", e, "floor", floor)
        assert e < max(2e-3, 2.5 * floor), (k, e, floor)
        checked += 1
    assert checked == 4 * 2 + 2 + 4 * 2 + 1


def ragged_case(H, drop_out=0.0, seed=11):
    """B = 2, R = 5, S = 9: 225 points per image, seven full tiles and a partial one."""
    meta = dict(fov=49.134342641202636, ray_start=0.25, ray_end=1.95, noise=0.0, clamp="softplus", white_back=True, last_back=False)
    B, R, S = 2, 5, 9
    gen = GL.fresh_generator(H, seed=seed, drop_out=drop_out)
    gt = torch.Generator().manual_seed(seed + 1)
    z = torch.randn(B, 32, generator=gt)
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix, sample_camera_positions
    np.random.seed(seed)
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y")
    rng = {"u_strat": torch.rand(B, R * R, S, generator=gt), "u_fine": torch.rand(B, R * R, S, generator=gt)}
    return gen, meta, z, cam, rng, B, R, S


def restatement_grads(gen, meta, z, cam, rng, R, S, loss, dtype, fine_z, drop=None):
    p = GL.cast_params(gen.siren, dtype, True)
    zz = z.detach().clone().to(dtype).requires_grad_(True)
    px, dp, aux = GL.render(p, zz, cam, meta, rng["u_strat"], rng["u_fine"], forced_fine_z=fine_z, drop=drop, R=R, S=S)
    grads = torch.autograd.grad(loss(px, dp), list(p.values()) + [zz])
    out = {"siren." + k: v.double().numpy() for k, v in zip(p, grads[:-1])}
    out["z"] = grads[-1].double().numpy()
    return out, aux


def test_render_backward_ragged_tiles_vs_float64(dev):
    """H = 256, 225 points per image: both backward precisions against autograd of the fp32 restatement, floor from its float64
    run.  The fine depths are the fp32 GPU forward's own, forced into every run (the field is chaotic in position)."""
    gen, meta, z, cam, rng, B, R, S = ragged_case(256)
    loss = random_weight_loss(B, R)
    on_gpu(gen, dev)
    set_precision(gen, "fp32")
    aux = {}
    with torch.no_grad():
        gen(z.to(dev), cam.to(dev), R, meta["fov"], meta["ray_start"], meta["ray_end"], S, True, _rng={k: v.to(dev) for k, v in rng.items()}, _aux=aux,
            **render_kwargs(meta))
    fz = aux["fine_z"].cpu()
    got = {}
    for bprec in ("fp32", "fp16"):
        set_precision(gen, bprec)
        got[bprec] = gpu_render_grads(gen, meta, z, cam, dict(rng, fine_z=fz), dev, R, S, loss)[0]
        if bprec == "fp16":
            from cnerf_amd import ops
            assert int(ops.LAST_SATURATED.item()) == 0
    gen.cpu()
    want, _ = restatement_grads(gen, meta, z, cam, rng, R, S, loss, torch.float32, fz)
    exact, _ = restatement_grads(gen, meta, z, cam, rng, R, S, loss, torch.float64, fz)
    for bprec in ("fp32", "fp16"):
        check_grads("ragged backward", got[bprec], want, exact, bprec)


@pytest.mark.parametrize("H", [64, 256])
def test_query_gradients(dev, H):
    """gen.siren(points, z) with B = 2, n = 4099: gradients of every parameter, z and the points against autograd of the
    restatement.  Without a volume there is no clamp: points outside the 1.2 cube have a non-zero position gradient."""
    gen = GL.fresh_generator(H, seed=3)
    gt = torch.Generator().manual_seed(4)
    B, n = 2, 4099
    z, pts, w = torch.randn(B, 32, generator=gt), (torch.rand(B, n, 3, generator=gt) * 2 - 1) * 0.75, torch.randn(B, n, 4, generator=gt)
    res = {}
    for dtype in (torch.float32, torch.float64):
        p = GL.cast_params(gen.siren, dtype, True)
        zz, pp = z.detach().clone().to(dtype).requires_grad_(True), pts.detach().clone().to(dtype).requires_grad_(True)
        grads = torch.autograd.grad((GL.field(p, zz, pp) * w.to(dtype)).sum(), list(p.values()) + [zz, pp])
        res[dtype] = {**{k: v.double().numpy() for k, v in zip(p, grads)}, "z": grads[-2].double().numpy(), "points": grads[-1].double().numpy()}
    want, exact = res[torch.float32], res[torch.float64]
    on_gpu(gen, dev)
    far = (pts.abs() > 0.6).any(-1).numpy()
    assert far.any()
    for bprec in ("fp32", "fp16"):
        set_precision(gen, bprec)
        gen.zero_grad()
        zd, pd = z.to(dev).requires_grad_(True), pts.to(dev).requires_grad_(True)
        (gen.siren(pd, zd) * w.to(dev)).sum().backward()
        torch.cuda.synchronize()
        got = {k: q.grad.double().cpu().numpy() for k, q in gen.siren.named_parameters()}
        got.update(z=zd.grad.double().cpu().numpy(), points=pd.grad.double().cpu().numpy())
        check_grads(f"query H={H}", got, want, exact, bprec)
        assert np.all(np.abs(got["points"][far]).sum(-1) > 0)


def test_backward_does_not_depend_on_the_chunking(dev, monkeypatch):
    """One image per chunk (ops.backward_chunk patched, and seen to be called) gives the gradients of all images in one chunk;
    tolerance of test_dropout_decisions_do_not_depend_on_the_chunking."""
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    gen, meta, z, cam, rng, B, R, S = ragged_case(64, seed=21)
    loss = random_weight_loss(B, R)
    on_gpu(gen, dev)
    real_chunk, seen = ops.backward_chunk, []

    def by_image(cfg, code, nb_max, have_act16, d):
        need = C.c_size_t(0)
        L.check(L.lib().cnerf_backward_workspace_bytes(C.byref(cfg), code, 1, 0, C.byref(need)), "cnerf_backward_workspace_bytes")
        seen.append(nb_max)
        return 1, need.value
    res = []
    for chunk in (real_chunk, by_image):
        monkeypatch.setattr(ops, "backward_chunk", chunk)
        res.append(gpu_render_grads(gen, meta, z, cam, rng, dev, R, S, loss)[0])
    monkeypatch.setattr(ops, "backward_chunk", real_chunk)
    assert seen == [B]
    for k in res[0]:
        assert scaled_err(res[1][k], res[0][k]) < 1e-5, k


def test_dropout(dev):
    """fp32, drop_out = 0.25, training mode.  Injected keep bytes (oracle.philox.dropout_keep, streams 4 and 5) reproduce the
    in-kernel Philox run bit for bit; the gradients match the restatement under those decisions."""
    from oracle import philox
    p = 0.25
    gen, meta, z, cam, rng, B, R, S = ragged_case(64, drop_out=p, seed=31)
    H, npts = 64, B * R * R * S
    loss = random_weight_loss(B, R)
    on_gpu(gen, dev, train=True)
    key = (4242, 7)
    keep = {s: torch.from_numpy(philox.dropout_keep(key[0], key[1], s, npts, GL.N_LAYERS, H, p)).reshape(GL.N_LAYERS, B, R * R * S, H) for s in (4, 5)}
    runs = []
    for r in (dict(rng, drop=(p, key)), dict(rng, drop=(p, key), drop_coarse=keep[4], drop_fine=keep[5])):
        aux = {}
        with torch.no_grad():
            px, dp = gen(z.to(dev), cam.to(dev), R, meta["fov"], meta["ray_start"], meta["ray_end"], S, True, _rng={k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in r.items()},
                         _aux=aux, **render_kwargs(meta))
        runs.append((px.cpu(), dp.cpu(), aux["coarse_rgb_sigma"].cpu(), aux["fine_rgb_sigma"].cpu(), aux["fine_z"].cpu()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert not torch.equal(runs[0][2], torch.zeros_like(runs[0][2]))
    fz = runs[0][4]
    gen.zero_grad()
    zd = z.to(dev).requires_grad_(True)
    px, dp = gen(zd, cam.to(dev), R, meta["fov"], meta["ray_start"], meta["ray_end"], S, True,
                 _rng={"u_strat": rng["u_strat"].to(dev), "u_fine": rng["u_fine"].to(dev), "fine_z": fz.to(dev), "drop": (p, key)}, **render_kwargs(meta))
    loss(px, dp).backward()
    torch.cuda.synchronize()
    got = {k: q.grad.double().cpu().numpy() for k, q in gen.named_parameters()}
    got["z"] = zd.grad.double().cpu().numpy()
    gen.cpu()
    want, aux32 = restatement_grads(gen, meta, z, cam, rng, R, S, loss, torch.float32, fz, drop=(p, keep[4], keep[5]))
    exact, _ = restatement_grads(gen, meta, z, cam, rng, R, S, loss, torch.float64, fz, drop=(p, keep[4], keep[5]))
    assert rgb_sigma_err(runs[0][2].numpy(), aux32["coarse_rgb_sigma"].detach().numpy()) < TOL
    for k, wv in want.items():
        floor, e = scaled_err(wv, exact[k]), scaled_err(got[k], wv)
        print("dropout backward", k, "err", e, "floor", floor)
        assert e < max(2e-3, 2.5 * floor), (k, e, floor)


def test_determinism(dev):
    """Three launches of the fp16x3 forward and of the fp16 backward on the H = 256 case: rgb_sigma of both passes is bit-identical,
    and so are the pixels and depths of the three forwards that keep their activations for the backward; the gradients (whose
    per-image weight reductions add with float atomics) agree to the tolerance of the chunking test."""
    gen, meta, z, cam, rng, B, R, S = ragged_case(256)
    loss = random_weight_loss(B, R)
    on_gpu(gen, dev)
    set_precision(gen, "fp16")
    outs, grads, imgs = [], [], []
    for _ in range(3):
        aux = {}
        with torch.no_grad():
            gen(z.to(dev), cam.to(dev), R, meta["fov"], meta["ray_start"], meta["ray_end"], S, True, _rng={k: v.to(dev) for k, v in rng.items()}, _aux=aux,
                **render_kwargs(meta))
        outs.append((aux["coarse_rgb_sigma"].cpu(), aux["fine_rgb_sigma"].cpu()))
        gr, px, dp = gpu_render_grads(gen, meta, z, cam, rng, dev, R, S, loss)
        grads.append(gr)
        imgs.append((px, dp))
    for im in imgs[1:]:
        assert torch.equal(im[0], imgs[0][0]) and torch.equal(im[1], imgs[0][1])
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    for gr in grads[1:]:
        for k in ("siren.network.0.layer.weight", "siren.network.3.layer.bias", "siren.final_layer.weight", "z"):
            assert scaled_err(gr[k], grads[0][k]) < 1e-5, k


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI alone: vols = NULL, grad_vols = NULL
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,bprec", [("fp32", "fp32"), ("fp16x3", "fp16")])
def test_ctypes_only_render_and_backward(dev, prec, bprec):
    """cnerf_pack_field, cnerf_render_forward and cnerf_render_backward through ctypes with NULL volumes and NULL gradient volumes,
    fp32 / fp32 and fp16x3 / fp16, against the fixture's gradients of the layer parameters and of freq / phase chained through
    the mapping MLP to z (fp32: scaled error < 2e-3; fp16: relative L2 < 3e-3 and scaled error < 5e-2)."""
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    g = fx("aux_shortsiren_small")
    m = g.meta
    B, R, S, H = m["B"], m["R"], m["S"], m["H"]
    P = R * R
    gen = on_gpu(GL.make_generator(g), dev)
    net = gen.siren
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L, cfg.n_levels = B, R, S, 0, 0, H, 4, 0
    cfg.ray_start, cfg.ray_end, cfg.voxel_length, cfg.fov_deg = m["ray_start"], m["ray_end"], 1.2, m["fov"]
    cfg.flags = L.F_NO_VOLUME | L.F_SIGMOID_RGB | L.F_HIERARCHICAL | L.F_WHITE_BACK
    cfg.precision = L.PREC_CODE[prec]
    bcode = L.PREC_CODE[bprec]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    L.check(lib.cnerf_workspace_bytes(C.byref(cfg), C.byref(a), C.byref(b), C.byref(c)), "workspace_bytes")
    assert b.value == 0
    params = [p.detach().contiguous() for p in net.field_params()]
    fp, gp = L.FieldParams(), L.FieldParamGrads()
    grads = [torch.zeros_like(p) for p in params]
    for i in range(4):
        fp.w[i], fp.b[i] = params[2 * i].data_ptr(), params[2 * i + 1].data_ptr()
        gp.w[i], gp.b[i] = grads[2 * i].data_ptr(), grads[2 * i + 1].data_ptr()
    fp.w_final, fp.b_final = params[8].data_ptr(), params[9].data_ptr()
    gp.w_final, gp.b_final = grads[8].data_ptr(), grads[9].data_ptr()
    f32 = dict(dtype=torch.float32, device=dev)
    packed = torch.empty(a.value // 4, **f32)
    L.check(lib.cnerf_pack_field(C.byref(cfg), C.byref(fp), L.ptr(packed), stream), "pack_field")
    nb = C.c_size_t()
    if bprec == "fp32":
        L.check(lib.cnerf_backward_bytes(C.byref(cfg), C.byref(nb)), "backward_bytes")
        packed_t = torch.empty(nb.value // 4, **f32)
        L.check(lib.cnerf_pack_field_transposed(C.byref(cfg), C.byref(fp), L.ptr(packed_t), stream), "pack_field_transposed")
    else:
        L.check(lib.cnerf_backward16_bytes(C.byref(cfg), C.byref(nb)), "backward16_bytes")
        packed_t = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        L.check(lib.cnerf_pack_field_chain16(C.byref(cfg), C.byref(fp), L.ptr(packed_t), stream), "pack_field_chain16")
    sat = torch.zeros(1, dtype=torch.int32, device=dev)
    z = T(g["z"], dev).requires_grad_(True)
    freq, phase = net.film(z)
    fr, ph = freq.detach().contiguous(), phase.detach().contiguous()
    cam = T(g["cam2worlds"], dev)
    u_strat, u_fine, fine_z = T(g["u_strat"], dev), T(g["u_fine"], dev), T(g["fine_z"], dev)
    rng = L.Rng()
    rng.u_strat, rng.u_fine, rng.fine_z = u_strat.data_ptr(), u_fine.data_ptr(), fine_z.data_ptr()
    ws = torch.empty(c.value, dtype=torch.uint8, device=dev)
    pixels, depth = torch.empty(B, 3, R, R, **f32), torch.empty(B, R, R, **f32)
    aux = L.Aux()
    c_rs, f_rs, c_z = torch.empty(B, P, S, 4, **f32), torch.empty(B, P, S, 4, **f32), torch.empty(B, P, S, **f32)
    aux.coarse_rgb_sigma, aux.fine_rgb_sigma, aux.coarse_z = c_rs.data_ptr(), f_rs.data_ptr(), c_z.data_ptr()
    L.check(lib.cnerf_render_forward(C.byref(cfg), None, L.ptr(packed), L.ptr(fr), L.ptr(ph), L.ptr(cam), C.byref(rng), L.ptr(pixels), L.ptr(depth),
                                     C.byref(aux), L.ptr(ws), stream), "render_forward")
    torch.cuda.synchronize()
    assert scaled_err(pixels.cpu().numpy(), g["pixels"]) <= TOL and scaled_err(depth.cpu().numpy(), g["depth"]) <= TOL
    px = pixels.clone().requires_grad_(True)
    dp = depth.clone().requires_grad_(True)
    random_weight_loss(B, R)(px, dp).backward()
    L.check(lib.cnerf_backward_workspace_bytes(C.byref(cfg), bcode, B, 0, C.byref(nb)), "backward_workspace_bytes")
    bws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    g_freq, g_phase = torch.zeros_like(fr), torch.zeros_like(ph)
    sv = L.Saved()
    sv.coarse_rgb_sigma, sv.coarse_z, sv.fine_rgb_sigma, sv.fine_z = c_rs.data_ptr(), c_z.data_ptr(), f_rs.data_ptr(), fine_z.data_ptr()
    L.check(lib.cnerf_render_backward(C.byref(cfg), bcode, B, None, C.byref(fp), L.ptr(packed), L.ptr(packed_t), L.ptr(fr), L.ptr(ph), L.ptr(cam),
                                      C.byref(rng), C.byref(sv), None, L.ptr(px.grad.contiguous()), L.ptr(dp.grad.contiguous()), C.byref(gp), L.ptr(g_freq),
                                      L.ptr(g_phase), None, L.ptr(sat), L.ptr(bws), stream), "render_backward")
    torch.cuda.synchronize()
    assert int(sat.item()) == 0

    def ok(k, mine, want):
        e, l2 = scaled_err(mine, want), rel_l2(mine, want)
        print("ctypes", prec, bprec, k, "err", e, "rel l2", l2)
        assert (e < 2e-3) if bprec == "fp32" else (l2 < 3e-3 and e < 5e-2), (k, e, l2)

    names = [f"siren.network.{i}.layer.{p}" for i in range(4) for p in ("weight", "bias")] + ["siren.final_layer.weight", "siren.final_layer.bias"]
    for k, gr in zip(names, grads):
        ok(k, gr.cpu().numpy(), g["grad/" + k])
    torch.autograd.backward([freq, phase], [g_freq, g_phase])
    ok("z", z.grad.cpu().numpy(), g["grad_z"])


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
def test_gan_step(dev):
    """One real D step and one G step of GanTrainer in the point-cloud setting: losses finite; generator, mapping-network and
    PointNet parameters all change."""
    from cnerf_amd.training import GanTrainer, default_metadata
    from cnerf_amd.training.gan_step import synthetic_sample
    torch.manual_seed(0)
    np.random.seed(0)
    md = default_metadata(img_size=16, num_steps=8, batch_size=2, batch_split=1, siren_type="SHORTSIREN", hidden_dim=64)
    tr = GanTrainer(md, dev)
    with torch.no_grad():
        tr.generator.siren.final_layer.weight[3] *= 30
    sample = synthetic_sample(2, 16, 8, dev, torch.Generator().manual_seed(1), pcl_points=64)
    watch = {"layer": tr.generator.siren.network[1].layer.weight, "layer0": tr.generator.siren.network[0].layer.weight,
             "head": tr.generator.siren.final_layer.weight, "mapping_first": tr.generator.siren.mapping_network.network[0].weight,
             "mapping_last": tr.generator.siren.mapping_network.network[6].weight, "pointnet_in": tr.encoder.fc_pos.weight,
             "pointnet_out": tr.encoder.fc_c.weight}
    before = {k: v.detach().clone() for k, v in watch.items()}
    tr.step(sample)
    torch.cuda.synchronize()
    for k in ("d", "g", "photo"):
        assert np.isfinite(tr.losses[k][-1]), k
    assert np.isfinite(tr.last["z_reg"]) and tr.last["z_reg"] > 0
    for k, v in watch.items():
        assert torch.isfinite(v).all() and not torch.equal(v.detach(), before[k]), k
