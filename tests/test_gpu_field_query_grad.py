"""Gradients of a field query, generator.siren(points, z) (ops.FieldQueryFunction -> cnerf_field_query_backward), against autograd
through the CPU oracle (oracle.render_oracle.field_eval) on the same inputs: every field parameter, every volume level, the global
feature and the query points, for the loss sum(w * rgb_sigma) with random w.

Yardstick of tests/test_gpu_parity.py::_ragged_backward_case: the fp32 oracle is the target and its float64 run sets the floor --
fp32 backward: scaled error < max(2e-3, 2.5 x floor); fp16 backward: relative L2 < max(3e-3, 2.5 x the oracle's own fp32-vs-float64
L2) -- the fp16 bound of tests/test_gpu_abi_only.py: a query of 2 x 4099 points averages fewer fp16 roundings than a render (measured
2.1e-3 on SHORTSIREN_FRes's layer-0 bias at H = 256) -- and scaled error < max(5e-2, 2.5 x floor).  Points are drawn over [-0.75, 0.75]^3, so a share lies outside the volume's
[-0.6, 0.6]^3 where the border clamp gives zero gradient; every point keeps 1e-3 voxel from a cell face and from the clamp bounds
of every level (d/dx jumps there)."""
import numpy as np
import pytest
import torch

from conftest import scaled_err

pytestmark = pytest.mark.gpu

VARIANTS = ["SHORTSIREN_FG", "SHORTSIREN_FG_Pyrmd", "SHORTSIREN_FRes", "TALLSIREN_dgx", "TALLSIREN"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def level_shapes(variant, V):
    """(channels, edge) per volume level."""
    return [(32, V), (64, max(V // 2, 2)), (32, max(V // 4, 2))] if variant.endswith("Pyrmd") else [(32, V)]


def query_points(B, n, edges, seed):
    """(B,n,3) in [-0.75, 0.75]^3, each coordinate >= 1e-3 voxel away from a cell face / clamp bound of every level."""
    g = torch.Generator().manual_seed(seed)
    out = torch.empty(0, 3)
    while out.shape[0] < B * n:
        p = (torch.rand(4 * B * n, 3, generator=g) * 2 - 1) * 0.75
        ok = torch.ones(p.shape[0], dtype=torch.bool)
        for V in edges:
            ic = ((p.double() / 0.6 + 1) * V - 1) / 2
            frac = ic - torch.floor(ic)
            ok &= ((frac > 1e-3) & (frac < 1 - 1e-3)).all(-1)
        out = torch.cat([out, p[ok]])
    return out[:B * n].reshape(B, n, 3).contiguous()


def make_case(variant, H, B=2, n=4099, V=8, drop_p=0.0, seed=0):
    from cnerf_amd.generators import ImplicitGenerator3d
    from cnerf_amd.generators.siren import FIELD_SPECS
    torch.manual_seed(seed)
    lv = level_shapes(variant, V)
    Z = 32
    c_in = sum(c for c, _ in lv)
    if variant == "TALLSIREN":
        gen = ImplicitGenerator3d(variant, 32, 3, 4, H, drop_out=drop_p)
    else:
        k0 = c_in + (3 if variant == "TALLSIREN_dgx" else 0)
        gen = ImplicitGenerator3d(variant, Z if FIELD_SPECS[variant].has_global else c_in, k0, 4, H, drop_out=drop_p)
    with torch.no_grad():
        gen.siren.final_layer.weight[3] *= 20
    has_glob = variant != "TALLSIREN" and FIELD_SPECS[variant].has_global
    vols = [torch.randn(B, c, e, e, e) * 0.5 for c, e in lv]
    glob = torch.randn(B, Z) if has_glob else None
    pts = query_points(B, n, [e for _, e in lv], seed + 1)
    w = torch.randn(B, n, 4)
    return gen, vols, glob, pts, w


def oracle_grads(variant, gen, vols, glob, pts, w, dtype, drop=None):
    """Autograd through the oracle: {name: gradient} over parameters, volume levels, global feature and points."""
    from oracle import render_oracle as O
    c = lambda t: t.detach().clone().to(dtype)
    params = {k: c(v).requires_grad_(True) for k, v in gen.siren.state_dict().items()}
    vr = [c(v).requires_grad_(True) for v in vols]
    gr = c(glob).requires_grad_(True) if glob is not None else None
    pr = c(pts).requires_grad_(True)
    torch.set_default_dtype(dtype)
    try:
        out, _ = O.field_eval(O.FIELD_SPECS[variant], params, vr if len(vr) > 1 else vr[0], gr, pr,
                              drop=None if drop is None else (drop[0], drop[1].to(dtype)))
        loss = (out * c(w)).sum()
        leaves = list(params.values()) + vr + ([gr] if gr is not None else []) + [pr]
        grads = torch.autograd.grad(loss, leaves)
    finally:
        torch.set_default_dtype(torch.float32)
    names = list(params.keys()) + [f"volume{i}" for i in range(len(vr))] + (["global_feature"] if gr is not None else []) + ["points"]
    return {k: g.double().numpy() for k, g in zip(names, grads)}


def gpu_grads(gen, vols, glob, pts, w, dev, backward_precision):
    """gen.siren(points, z) and its gradients on the GPU, same names as oracle_grads."""
    from cnerf_amd import ops
    net = gen.siren
    net.precision = "fp32" if backward_precision == "fp32" else "fp16x3"
    net.backward_precision = backward_precision
    net.zero_grad()
    vd = [v.to(dev).requires_grad_(True) for v in vols]
    gd = glob.to(dev).requires_grad_(True) if glob is not None else None
    pd = pts.to(dev).requires_grad_(True)
    fv = vd if len(vd) > 1 else vd[0]
    out = net(pd, (fv, gd) if gd is not None else fv)
    (out * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    if backward_precision == "fp16":
        assert int(ops.LAST_SATURATED.item()) == 0, "fp16 gradients were clamped"
    got = {k: p.grad for k, p in net.named_parameters()}
    got.update({f"volume{i}": v.grad for i, v in enumerate(vd)})
    if gd is not None:
        got["global_feature"] = gd.grad
    got["points"] = pd.grad
    return {k: g.double().cpu().numpy() for k, g in got.items()}


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("variant", VARIANTS)
def test_query_gradients_vs_oracle_autograd(dev, variant, H):
    gen, vols, glob, pts, w = make_case(variant, H)
    want = oracle_grads(variant, gen, vols, glob, pts, w, torch.float32)
    exact = oracle_grads(variant, gen, vols, glob, pts, w, torch.float64)
    ext = [p.abs().max().item() for p in pts.unbind(-1)]
    assert max(ext) > 0.6, "some points must lie outside the volume"
    outside = (pts.abs() > 0.6).any(-1)
    gen.to(dev)
    gen.set_device(dev)
    gen.eval()
    for bprec in ("fp32", "fp16"):
        got = gpu_grads(gen, vols, glob, pts, w, dev, bprec)
        assert set(got) == set(want), (set(got) ^ set(want))
        for k, wv in want.items():
            floor = scaled_err(wv, exact[k])
            e, l2 = scaled_err(got[k], wv), rel_l2(got[k], wv)
            if bprec == "fp32":
                assert e < max(2e-3, 2.5 * floor), (variant, H, bprec, k, e, floor)
            else:
                assert l2 < max(3e-3, 2.5 * rel_l2(wv, exact[k])) and e < max(5e-2, 2.5 * floor), (variant, H, bprec, k, e, l2, floor)
        # beyond the clamp of every level the lookup term is zero on that axis: what remains there is the xyz input's
        if variant not in ("TALLSIREN", "TALLSIREN_dgx"):
            far = (pts.abs() > 0.6)
            assert far.any()
            assert np.all(got["points"][far.numpy()] == 0.0)
        assert outside.any()


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "TALLSIREN"])
def test_query_gradients_with_dropout(dev, variant):
    """Training mode, fp32, drop_out > 0: the forward's keep decisions (Philox stream 6, oracle.philox.dropout_keep) reach the
    backward, whichever way it chunks."""
    from oracle import philox
    H, p = 64, 0.25
    gen, vols, glob, pts, w = make_case(variant, H, n=1500, drop_p=p, seed=5)
    gen.to(dev)
    gen.set_device(dev)
    gen.train()
    seed, offset = torch.cuda.initial_seed(), gen.siren._drop_calls
    got = gpu_grads(gen, vols, glob, pts, w, dev, "fp32")
    assert gen.siren._drop_calls == offset + 1
    B, n = pts.shape[:2]
    n_drop = sum(1 for k in gen.siren.spec.layers if k != "res")
    keep = torch.from_numpy(philox.dropout_keep(seed, offset, 6, B * n, n_drop, H, p)).reshape(n_drop, B, n, H)
    gen.cpu()
    want = oracle_grads(variant, gen, vols, glob, pts, w, torch.float32, drop=(p, keep))
    exact = oracle_grads(variant, gen, vols, glob, pts, w, torch.float64, drop=(p, keep))
    for k, wv in want.items():
        floor = scaled_err(wv, exact[k])
        e = scaled_err(got[k], wv)
        assert e < max(2e-3, 2.5 * floor), (variant, k, e, floor)


@pytest.mark.parametrize("variant,bprec,drop_p", [("SHORTSIREN_FG", "fp32", 0.25), ("TALLSIREN", "fp32", 0.25), ("SHORTSIREN_FG_Pyrmd", "fp16", 0.0),
                                                 ("TALLSIREN", "fp16", 0.0)])
def test_query_gradients_do_not_depend_on_the_chunking(dev, monkeypatch, variant, bprec, drop_p):
    """ops.query_chunk forced to ragged 1000-point chunks (4099 points per image: four full chunks and a 99-point tail) gives the
    gradients of one chunk per image: dropout decisions offset by the point's index in the whole call (a wrong offset moves every
    gradient by O(1)), sums in another order (fp32: 1e-4 scaled -- TALLSIREN's mapping-weight GEMM over 8198 points cancels to
    2.5e-5 -- fp16: per-chunk gradient scales, a few fp16 roundings apart)."""
    from cnerf_amd import ops
    gen, vols, glob, pts, w = make_case(variant, 64, drop_p=drop_p, seed=11)
    gen.to(dev)
    gen.set_device(dev)
    real = ops.query_chunk
    seen = []

    def ragged(n, bytes_of, d):
        seen.append(n)
        return 1000, bytes_of(1000)
    res = []
    for chunk in (real, ragged):
        monkeypatch.setattr(ops, "query_chunk", chunk)
        if drop_p:
            gen.train()
            gen.siren._drop_calls = 7           # same keep decisions in both runs
        else:
            gen.eval()
        res.append(gpu_grads(gen, vols, glob, pts, w, dev, bprec))
    monkeypatch.setattr(ops, "query_chunk", real)
    assert seen == [pts.shape[1]], "the chunk-size patch was not applied"
    for k in res[0]:
        if bprec == "fp32":
            assert scaled_err(res[1][k], res[0][k]) < 1e-4, (k, scaled_err(res[1][k], res[0][k]))
        else:
            assert rel_l2(res[1][k], res[0][k]) < 2e-3, (k, rel_l2(res[1][k], res[0][k]))


def test_no_grad_query_is_unchanged_and_losses_add(dev):
    """Under no_grad the query is the plain forward -- bit-equal to the output of the differentiable one; a render loss plus a query
    loss in one backward() gives the sum of the two separate gradients."""
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    gen, vols, glob, pts, w = make_case("SHORTSIREN_FG", 64, n=777, seed=21)
    gen.to(dev)
    gen.set_device(dev)
    gen.eval()
    net = gen.siren
    fv, gl, pd, wd = vols[0].to(dev), glob.to(dev), pts.to(dev), w.to(dev)
    with torch.no_grad():
        plain = net(pd, (fv, gl))
    assert plain.grad_fn is None
    fvg = fv.clone().requires_grad_(True)
    diff = net(pd, (fvg, gl))
    assert diff.grad_fn is not None
    assert torch.equal(plain, diff.detach())

    B, R, S = pts.shape[0], 8, 12
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y").to(dev)
    torch.manual_seed(3)
    rng = {"u_strat": torch.rand(B, R * R, S, device=dev), "u_fine": torch.rand(B, R * R, S, device=dev)}

    def grads(render, query):
        gen.zero_grad()
        f, g = fv.clone().requires_grad_(True), gl.clone().requires_grad_(True)
        loss = 0.0
        if render:
            px, dp = gen((f, g), cam, R, 49.13, 0.25, 1.95, S, True, clamp_mode="relu", nerf_noise=0.0, white_back=True, _rng=dict(rng))
            loss = loss + px.square().mean() + dp.mean()
        if query:
            loss = loss + (net(pd, (f, g)) * wd).sum() * 1e-3
        loss.backward()
        out = {k: p.grad.clone() for k, p in gen.named_parameters() if p.grad is not None}
        out.update(volume=f.grad.clone(), global_feature=g.grad.clone())
        return out
    a, b, both = grads(True, False), grads(False, True), grads(True, True)
    for k in both:
        s = a.get(k, 0) + b.get(k, 0)
        assert scaled_err(both[k].cpu().numpy(), s.cpu().numpy()) < 1e-5, k
