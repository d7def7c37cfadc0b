"""cnerf_pfilm_backward_finish: the mapping-network stage of the per-point FiLM family's exact fp32 backward (csrc/pfilm_finish.hip).
1. the stage alone on synthetic chunk buffers against the same formulas in float64, at the derived dot-product bound;
2. forward + exact backward of the TALLSIREN fixtures through ctypes ALONE, the backward spelled with stage calls and as one
   cnerf_render_backward call, against the reference's autograd;
3. the PyTorch mirror: one cnerf_render_backward call whatever the chunking, no stage call from Python."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import scaled_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24           # unit roundoff of fp32
V = 5                    # side of the stage test's feature volume
CANARY = 4               # rows of 1e30 behind row n of every input


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def dptr(t):
    if t is None:
        return C.c_void_p(None)
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def pfilm_cfg(L, H, nl, V, precision="fp32"):
    cfg = L.Cfg()
    cfg.B, cfg.V, cfg.C, cfg.H, cfg.L = 1, V, 32, H, nl
    for i in range(nl):
        cfg.layer_kind[i] = L.LAYER_PFILM
    cfg.voxel_length = 1.2
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, V, 32
    cfg.precision = L.PREC_CODE[precision]
    return cfg


def within(got, want, bound, what):
    """|got - want| <= bound elementwise (float64 on the CPU); a zero bound demands equality."""
    got, want, bound = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, np.float64) for t in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), what
    excess = np.abs(got - want) - bound
    i = np.unravel_index(np.argmax(excess), excess.shape)
    print(f"{what:24s} max |err| / bound {np.max(np.abs(got - want) / np.maximum(bound, 1e-300)):.3f}")
    assert excess[i] <= 0, (what, i, got[i], want[i], bound[i])


def dot_bound(k, A, B):
    """(k + 2) 2^-24 |A|^T |B|: the rounding of a length-k fp32 dot product summed in any order (k - 1 additions and one rounding per
    product, fused or not; one spare for the LeakyReLU factor of g_mpre)."""
    return (k + 2) * U * (np.abs(A).T @ np.abs(B))


@pytest.mark.parametrize("n_images,npi,H,nl", [(1, 1, 64, 8), (2, 45, 64, 8), (1, 33, 128, 3), (3, 70, 256, 8)])
def test_stage_alone_against_float64(dev, n_images, npi, H, nl):
    """A single partial tile; ragged tiles across image boundaries; every width; 2 L H = 768, no multiple of 256.  Every output against
    the formulas of include/cnerf.h in float64, each within the dot-product bound of ITS OWN fp32 inputs -- the products behind dWm1 and
    d feat read the stage's g_mpre (the head of the workspace), which itself is held to the bound of G Wm2.  Rows of 1e30 behind row n of
    every input buffer must stay unread, bytes behind every output unwritten; a second call doubles what is accumulated."""
    import cnerf_amd
    from cnerf_amd.generators import siren
    L = cnerf_amd._lib
    lib = L.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc, what: (_ for _ in ()).throw(AssertionError(f"{what}: rc {rc}: {lib.cnerf_last_error().decode()}")) if rc else None
    torch.manual_seed(1000 * H + npi)
    n, K2 = n_images * npi, 2 * nl * H
    net = siren.TALLSIREN(3, 32, H)
    mp = net.mapping_network.network
    Wm1 = mp[0].weight.detach().clone()                                                         # (256, 32)
    Wm2 = torch.cat([mp[2].weight.detach()[:nl * H], mp[2].weight.detach()[8 * H:8 * H + nl * H]]).contiguous()   # (2 L H, 256): [f | p] of the first L layers

    # chunk buffers as cnerf_field_backward lays them out, CANARY rows of 1e30 behind the last row of each
    def with_canary(rows, width, head_floats=0, scale=1.0):
        t = torch.full((head_floats + (rows + CANARY) * width,), 1e30)
        t[:head_floats + rows * width] = torch.randn(head_floats + rows * width) * scale
        return t
    pts = with_canary(n, 3, scale=0.35)                       # some positions beyond the 1.2 cube's faces (clamped lookups)
    feat = with_canary(n, 32)
    a_h = with_canary(n, 256, head_floats=nl * n * H)         # y_0 .. y_{L-1}, then m
    a_g = with_canary(n, K2, head_floats=nl * n * H)          # g_pre_0 .. g_pre_{L-1}, then G
    go = with_canary(n, 4)
    m = a_h[nl * n * H:nl * n * H + n * 256].view(n, 256)
    m[1::3] = 0.0                                             # rows and columns exactly at the kink of the LeakyReLU: slope 0.2 there
    m[:, ::7] = 0.0
    assert (m < 0).any() and (m == 0).any() and (m > 0).any()
    d = {k: t.to(dev) for k, t in dict(pts=pts, feat=feat, a_h=a_h, a_g=a_g, go=go).items()}

    cfg = pfilm_cfg(L, H, nl, V)
    pm, wsb = C.c_size_t(), C.c_size_t()
    ok(lib.cnerf_pfilm_finish_bytes(C.byref(cfg), n_images, npi, C.byref(pm), C.byref(wsb)), "pfilm_finish_bytes")
    fp = L.FieldParams()
    Wm1_d, Wm2_d = Wm1.to(dev), Wm2.to(dev)
    fp.map_w1, fp.map_w2 = Wm1_d.data_ptr(), Wm2_d.data_ptr()
    packed_map = torch.empty(pm.value // 4, device=dev)
    ok(lib.cnerf_pack_pfilm_map_transposed(C.byref(cfg), C.byref(fp), dptr(packed_map), stream), "pack_pfilm_map_transposed")
    SENT = 12345.0
    ws = torch.full((wsb.value // 4 + 256,), SENT, device=dev)
    grad_feat = torch.full((n + CANARY, 32), SENT, device=dev)
    g_vol = torch.zeros((n_images + 1, V, V, V, 32), device=dev)
    g_vol[n_images] = SENT
    shapes = {"w0": (H, 3), "b0": (H,), **{f"w{l}": (H, H) for l in range(1, nl)}, **{f"b{l}": (H,) for l in range(1, nl)},
              "w_final": (4, H), "b_final": (4,), "map_w1": (256, 32), "map_b1": (256,), "map_w2": (K2, 256), "map_b2": (K2,)}
    grads = {k: torch.zeros(s, device=dev) for k, s in shapes.items()}
    gs = L.FieldParamGrads()
    for l in range(nl):
        gs.w[l], gs.b[l] = grads[f"w{l}"].data_ptr(), grads[f"b{l}"].data_ptr()
    for k in ("w_final", "b_final", "map_w1", "map_b1", "map_w2", "map_b2"):
        setattr(gs, k, grads[k].data_ptr())

    def call():
        ok(lib.cnerf_pfilm_backward_finish(C.byref(cfg), None, dptr(packed_map), n_images, npi, dptr(d["pts"]), dptr(d["feat"]), dptr(d["a_h"]),
                                           dptr(d["a_g"]), dptr(d["go"]), C.byref(gs), dptr(g_vol), dptr(grad_feat), dptr(ws), stream),
           "pfilm_backward_finish")
        torch.cuda.synchronize()
    call()
    once = {k: t.clone() for k, t in grads.items()}
    once_vol, once_feat = g_vol.clone(), grad_feat.clone()
    g_mpre = ws[:n * 256].view(n, 256).cpu().double().numpy()
    assert (ws[wsb.value // 4:] == SENT).all() and (grad_feat[n:] == SENT).all() and (g_vol[n_images] == SENT).all()

    # the same formulas in float64
    f64 = lambda t: t.double().numpy()
    y = f64(a_h[:nl * n * H].view(nl, n, H))
    gp = f64(a_g[:nl * n * H].view(nl, n, H))
    G = f64(a_g[nl * n * H:nl * n * H + n * K2].view(n, K2))
    m64, P, F, GO = f64(m), f64(pts[:n * 3].view(n, 3)), f64(feat[:n * 32].view(n, 32)), f64(go[:n * 4].view(n, 4))
    ones = np.ones((n, 1))
    slope = np.where(m64 > 0, 1.0, float(np.float32(0.2)))
    within(g_mpre, (G @ f64(Wm2)) * slope, dot_bound(K2, G.T, f64(Wm2)) * slope, "g_mpre")
    within(once_feat[:n], g_mpre @ f64(Wm1), dot_bound(256, g_mpre.T, f64(Wm1)), "grad_feat")
    expect = {"w0": (gp[0].T @ P, dot_bound(n, gp[0], P)), "w_final": (GO.T @ y[nl - 1], dot_bound(n, GO, y[nl - 1])),
              "b_final": (GO.sum(0), dot_bound(n, GO, ones)[:, 0]), "map_w2": (G.T @ m64, dot_bound(n, G, m64)),
              "map_b2": (G.sum(0), dot_bound(n, G, ones)[:, 0]), "map_w1": (g_mpre.T @ F, dot_bound(n, g_mpre, F)),
              "map_b1": (g_mpre.sum(0), dot_bound(n, g_mpre, ones)[:, 0])}
    for l in range(nl):
        expect[f"b{l}"] = (gp[l].sum(0), dot_bound(n, gp[l], ones)[:, 0])
        if l:
            expect[f"w{l}"] = (gp[l].T @ y[l - 1], dot_bound(n, gp[l], y[l - 1]))
    assert set(expect) == set(grads)
    for k, (want, bound) in expect.items():
        within(once[k], want, bound, k)

    # the volume: the addends of cnerf_scatter_features on the returned rows, in another order.  A voxel channel receives at most 8 addends
    # per point of its image (the corners of a clamped position can coincide): two orders of k addends differ by <= 2 (k - 1) u sum |addend|
    scfg = pfilm_cfg(L, H, nl, V)
    scfg.B = n_images
    want_vol, abs_vol = torch.zeros((n_images, V, V, V, 32), device=dev), torch.zeros((n_images, V, V, V, 32), device=dev)
    rows = once_feat[:n].contiguous()
    ok(lib.cnerf_scatter_features(C.byref(scfg), dptr(d["pts"]), npi, dptr(rows), dptr(want_vol), stream), "scatter_features")
    ok(lib.cnerf_scatter_features(C.byref(scfg), dptr(d["pts"]), npi, dptr(rows.abs()), dptr(abs_vol), stream), "scatter_features")
    torch.cuda.synchronize()
    assert want_vol.abs().max().item() > 0
    vol_bound = 2 * (8 * npi) * U * abs_vol.cpu().double().numpy()
    within(once_vol[:n_images], want_vol, vol_bound, "grad_fvol_cl")

    # accumulation: a second call adds the same sums, in whatever order, to what the first left: within the bound of the first call's own
    # value once more for the second sum, and once for adding its addends onto a base of that size
    call()
    for k, (want, bound) in expect.items():
        within(grads[k], 2 * once[k].cpu().double().numpy(), 4 * bound, "twice " + k)
    within(g_vol[:n_images], 2 * once_vol[:n_images].cpu().double().numpy(), 4 * vol_bound, "twice grad_fvol_cl")
    assert torch.equal(grad_feat, once_feat)
    assert (ws[wsb.value // 4:] == SENT).all() and (g_vol[n_images] == SENT).all()


@pytest.mark.parametrize("spelling", ["stages", "one_call_per_image", "one_call_all_images"])
@pytest.mark.parametrize("name", ["tallsiren_small", "tallsiren_drop_small"])
def test_exact_backward_through_ctypes_only(golden, dev, name, spelling):
    """tests/test_gpu_abi_only.py's forward + backward for this family in fp32: the render through cnerf_render_forward, the backward
    either spelled with stage calls -- cnerf_merge_composite_backward, then per pass cnerf_field_backward (one chunk of all images) and
    cnerf_pfilm_backward_finish on the sample positions cnerf_aux kept -- or as ONE cnerf_render_backward call with images_per_chunk 1
    or B, whose forward keeps no sample positions (the chunk's re-run writes them) -- no cnerf_amd.ops, no torch matmul.  The dropout
    fixture passes its keep bytes (cnerf_rng) and drop_p.  Against the reference's autograd at test_backward_teacher_forced's tolerance."""
    import cnerf_amd
    from test_gpu_parity import reference_grad_noise_floor
    L = cnerf_amd._lib
    lib = L.lib()
    g = golden(name)
    m = g.meta
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc, what: (_ for _ in ()).throw(AssertionError(f"{what}: rc {rc}: {lib.cnerf_last_error().decode()}")) if rc else None
    nl = 8
    B, R, S, H, Vf, Cc = m["B"], m["R"], m["S"], m["H"], g["feature_volume"].shape[-1], m["C"]
    assert m["variant"] == "TALLSIREN" and m["hierarchical"] and m["noise"] == 0
    P, npi = R * R, R * R * S
    n = B * npi
    prm = {k: T(v) for k, v in g.params().items()}

    cfg = pfilm_cfg(L, H, nl, Vf)
    cfg.B, cfg.R, cfg.S = B, R, S
    cfg.ray_start, cfg.ray_end, cfg.noise_std, cfg.fov_deg = m["ray_start"], m["ray_end"], m["noise"], m["fov"]
    cfg.flags = (L.F_HIERARCHICAL | (L.F_WHITE_BACK if m["white_back"] else 0) | (L.F_LAST_BACK if m["last_back"] else 0) |
                 (L.F_SOFTPLUS if m["clamp"] == "softplus" else 0))
    cfg.drop_p = float(m.get("drop_out", 0))

    fp, gp = L.FieldParams(), L.FieldParamGrads()
    grads = {k: torch.zeros_like(v) for k, v in prm.items()}
    for i in range(nl):
        fp.w[i], fp.b[i] = prm[f"network.{i}.layer.weight"].data_ptr(), prm[f"network.{i}.layer.bias"].data_ptr()
        gp.w[i], gp.b[i] = grads[f"network.{i}.layer.weight"].data_ptr(), grads[f"network.{i}.layer.bias"].data_ptr()
    for slot, key in (("w_final", "final_layer.weight"), ("b_final", "final_layer.bias"), ("map_w1", "mapping_network.network.0.weight"),
                      ("map_b1", "mapping_network.network.0.bias"), ("map_w2", "mapping_network.network.2.weight"),
                      ("map_b2", "mapping_network.network.2.bias")):
        setattr(fp, slot, prm[key].data_ptr())
        setattr(gp, slot, grads[key].data_ptr())

    fvol = T(g["feature_volume"])
    fcl = torch.empty((B, Vf, Vf, Vf, Cc), device=dev)
    ok(lib.cnerf_fvol_channel_last(B, Cc, Vf, dptr(fvol), dptr(fcl), stream), "channel_last")
    vols = L.Volumes()
    vols.level[0] = fcl.data_ptr()
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    ok(lib.cnerf_workspace_bytes(C.byref(cfg), C.byref(a), C.byref(b), C.byref(c)), "workspace_bytes")
    packed = torch.empty(a.value // 4, device=dev)
    ok(lib.cnerf_pack_field(C.byref(cfg), C.byref(fp), dptr(packed), stream), "pack_field")
    ws = torch.empty(c.value, dtype=torch.uint8, device=dev)

    rng = L.Rng()
    keep = {k: T(g[k]).reshape(B, P, -1).contiguous() for k in ("u_strat", "u_fine")}
    keep["fine_z"] = T(g["fine_z"]).reshape(B, P, S).contiguous()          # the reference's resampled depths, forced
    for k in ("drop_coarse", "drop_fine"):
        if g.get(k) is not None:
            keep[k] = T(g[k]).to(torch.uint8).contiguous()
    for k, t in keep.items():
        setattr(rng, k, t.data_ptr())
    aux = L.Aux()
    sv = {"coarse_rgb_sigma": torch.empty((B, P, S, 4), device=dev), "coarse_z": torch.empty((B, P, S), device=dev),
          "fine_rgb_sigma": torch.empty((B, P, S, 4), device=dev), "fine_z": torch.empty((B, P, S), device=dev)}
    if spelling == "stages":
        sv.update(coarse_points=torch.empty((B, P, S, 3), device=dev), fine_points=torch.empty((B, P, S, 3), device=dev))
    for k, t in sv.items():
        setattr(aux, k, t.data_ptr())
    cam = T(g["cam2worlds"]).reshape(B, 4, 4).contiguous()
    pixels, depth = torch.empty((B, 3, R, R), device=dev), torch.empty((B, R, R), device=dev)
    ok(lib.cnerf_render_forward(C.byref(cfg), C.byref(vols), dptr(packed), None, None, dptr(cam), C.byref(rng), dptr(pixels), dptr(depth),
                                C.byref(aux), dptr(ws), stream), "render_forward")
    assert scaled_err(pixels.cpu().numpy(), g["pixels"]) < 2e-4 and scaled_err(depth.cpu().numpy(), g["depth"]) < 2e-4
    grad_pixels = (2.0 * pixels / pixels.numel()).contiguous()              # loss = pixels.square().mean() + depth.mean()
    grad_depth = torch.full_like(depth, 1.0 / depth.numel())

    nb = C.c_size_t()
    ok(lib.cnerf_backward_bytes(C.byref(cfg), C.byref(nb)), "backward_bytes")
    packed_t = torch.empty(nb.value // 4, device=dev)
    ok(lib.cnerf_pack_field_transposed(C.byref(cfg), C.byref(fp), dptr(packed_t), stream), "pack_field_transposed")
    g_vol = torch.zeros_like(fcl)
    gvols = L.Volumes()
    gvols.level[0] = g_vol.data_ptr()
    if spelling == "stages":          # ---- the backward, stage by stage
        pm, fws = C.c_size_t(), C.c_size_t()
        ok(lib.cnerf_pfilm_finish_bytes(C.byref(cfg), B, npi, C.byref(pm), C.byref(fws)), "pfilm_finish_bytes")
        packed_map = torch.empty(pm.value // 4, device=dev)
        ok(lib.cnerf_pack_pfilm_map_transposed(C.byref(cfg), C.byref(fp), dptr(packed_map), stream), "pack_pfilm_map_transposed")
        finish_ws = torch.empty(fws.value, dtype=torch.uint8, device=dev)
        gc, gf = torch.empty((B, P, S, 4), device=dev), torch.empty((B, P, S, 4), device=dev)
        ok(lib.cnerf_merge_composite_backward(C.byref(cfg), dptr(sv["coarse_rgb_sigma"]), dptr(sv["coarse_z"]), dptr(sv["fine_rgb_sigma"]),
                                              dptr(keep["fine_z"]), None, dptr(grad_pixels), dptr(grad_depth), dptr(gc), dptr(gf), stream),
           "merge_composite_backward")
        act_feat, act_go = torch.empty((n, 32), device=dev), torch.empty((n, 4), device=dev)
        act_h = torch.empty(nl * n * H + n * 256, device=dev)
        act_c, act_g = torch.empty(3 * nl * n * H, device=dev), torch.empty(3 * nl * n * H, device=dev)
        for pss, g_out, saved_out, points, mask in ((0, gc, sv["coarse_rgb_sigma"], sv["coarse_points"], keep.get("drop_coarse")),
                                                    (1, gf, sv["fine_rgb_sigma"], sv["fine_points"], keep.get("drop_fine"))):
            ok(lib.cnerf_field_backward(C.byref(cfg), pss, 0, B, C.byref(vols), dptr(packed), dptr(packed_t), None, None, dptr(cam), dptr(keep["u_strat"]),
                                        dptr(keep["fine_z"]), dptr(g_out), dptr(saved_out), dptr(act_feat), dptr(act_h), dptr(act_c), dptr(act_g),
                                        dptr(act_go), C.byref(gvols), dptr(mask), stream), "field_backward")
            ok(lib.cnerf_pfilm_backward_finish(C.byref(cfg), C.byref(fp), dptr(packed_map), B, npi, dptr(points), dptr(act_feat), dptr(act_h), dptr(act_g),
                                               dptr(act_go), C.byref(gp), dptr(g_vol), None, dptr(finish_ws), stream), "pfilm_backward_finish")
    else:                             # ---- the backward in one call
        cnt = 1 if spelling == "one_call_per_image" else B
        ok(lib.cnerf_backward_workspace_bytes(C.byref(cfg), L.PREC_FP32, cnt, 0, C.byref(nb)), "backward_workspace_bytes")
        bws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        saved = L.Saved()
        saved.coarse_rgb_sigma, saved.coarse_z = sv["coarse_rgb_sigma"].data_ptr(), sv["coarse_z"].data_ptr()
        saved.fine_rgb_sigma, saved.fine_z = sv["fine_rgb_sigma"].data_ptr(), keep["fine_z"].data_ptr()
        ok(lib.cnerf_render_backward(C.byref(cfg), L.PREC_FP32, cnt, C.byref(vols), C.byref(fp), dptr(packed), dptr(packed_t), None, None, dptr(cam),
                                     C.byref(rng), C.byref(saved), None, dptr(grad_pixels), dptr(grad_depth), C.byref(gp), None, None, C.byref(gvols),
                                     None, dptr(bws), stream), "render_backward")
    gv_cf = torch.empty_like(fvol)
    ok(lib.cnerf_fvol_channel_first(B, Cc, Vf, dptr(g_vol), dptr(gv_cf), stream), "channel_first")
    torch.cuda.synchronize()

    floor = reference_grad_noise_floor(g)
    ref = g.grads()
    assert set(ref) == set(grads)
    for k, t in grads.items():
        e, tol = scaled_err(t.cpu().numpy(), ref[k]), max(2e-3, 2.5 * floor["siren." + k])
        print(f"{k:40s} {e:.2e} (tolerance {tol:.2e})")
        assert e < tol, (k, e, tol)
    e, tol = scaled_err(gv_cf.cpu().numpy(), g["grad_feature_volume"]), max(2e-3, 2.5 * floor["feature_volume"])
    assert e < tol, ("feature_volume", e, tol)


def test_mirror_is_one_call_whatever_the_chunking(dev, monkeypatch):
    """With ops.backward_chunk answering one image per chunk the mirror still makes ONE cnerf_render_backward call (images_per_chunk 1:
    3 images x 2 passes = 6 chunks inside the library) and no stage call of its own, and the gradients still meet the gates of
    _ragged_backward_case (autograd through the CPU oracle)."""
    import cnerf_amd
    from cnerf_amd import ops
    from test_gpu_parity import _ragged_backward_case
    L = cnerf_amd._lib
    lib = L.lib()
    calls = {k: [] for k in ("cnerf_render_backward", "cnerf_field_backward", "cnerf_pfilm_backward_finish")}

    def counting(name, real):
        def call(*args):
            calls[name].append(args)
            return real(*args)
        return call
    for name in calls:
        monkeypatch.setattr(lib, name, counting(name, getattr(lib, name)))

    def by_image(cfg, code, nb_max, have_act16, d):
        need = C.c_size_t(0)
        L.check(lib.cnerf_backward_workspace_bytes(C.byref(cfg), code, 1, 0, C.byref(need)), "cnerf_backward_workspace_bytes")
        return 1, need.value
    monkeypatch.setattr(ops, "backward_chunk", by_image)
    _ragged_backward_case(dev, dict(B=3, R=4, S=9, V=5, H=256), "TALLSIREN", "fp32")
    assert len(calls["cnerf_render_backward"]) == 1 and calls["cnerf_render_backward"][0][2] == 1          # images_per_chunk
    assert calls["cnerf_field_backward"] == [] and calls["cnerf_pfilm_backward_finish"] == []
