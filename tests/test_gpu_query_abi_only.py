"""A field query and its gradients driven through the C ABI ALONE: cnerf_field_forward, then cnerf_field_query_backward, with raw
device pointers -- no cnerf_amd.ops, no autograd.Function.  The module classes only draw the initial parameters; the FiLM mapping
Linear is the one piece the host evaluates (and differentiates) itself.  Gradients are compared with autograd through the CPU oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import scaled_err

pytestmark = pytest.mark.gpu


def dptr(t):
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("variant,fwd,bwd", [("SHORTSIREN_FG", "fp32", "fp32"), ("SHORTSIREN_FG_Pyrmd", "fp16x3", "fp16"), ("TALLSIREN", "fp16x3", "fp16"),
                                             ("TALLSIREN", "fp32", "fp32")])
def test_query_forward_and_backward_through_ctypes_only(variant, fwd, bwd):
    """3001 points per image in chunks of 1024: three chunks per image, the last one ragged.  TALLSIREN's exact fp32 backward (the
    per-point FiLM body of the one call: the stage kernels behind cnerf_field_query_backward): 4099 points in four 1000-point chunks
    and a 99-point tail, at the gate of the other fp32 row (rel l2 2e-3, scaled 2e-2 against autograd through the oracle)."""
    import cnerf_amd
    from cnerf_amd.generators import siren as S
    from oracle import render_oracle as O
    L = cnerf_amd._lib
    lib = L.lib()
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc, what: (_ for _ in ()).throw(AssertionError(f"{what}: rc {rc}: {lib.cnerf_last_error().decode()}")) if rc else None
    nul = C.c_void_p(None)
    p_or_null = lambda t: nul if t is None else dptr(t)
    torch.manual_seed(7)
    B, H, V, Z = 2, 64, 8, 32
    n, ppc = (4099, 1000) if (variant, bwd) == ("TALLSIREN", "fp32") else (3001, 1024)
    spec = O.FIELD_SPECS[variant]
    lv = [(32, V), (64, V // 2), (32, V // 4)] if spec.input == "pyramid" else [(32, V)]
    Cc = sum(c for c, _ in lv)
    net = S.TALLSIREN(3, 32, H) if variant == "TALLSIREN" else getattr(S, variant)(input_dim=Cc, z_dim=Z, hidden_dim=H)
    with torch.no_grad():
        net.final_layer.weight[3] *= 20
    prm = {k: v.detach().to(dev).contiguous() for k, v in net.state_dict().items()}
    vols = [torch.randn(B, c, e, e, e, device=dev) * 0.5 for c, e in lv]
    glob = torch.randn(B, Z, device=dev) if spec.has_global else None
    pts = ((torch.rand(B, n, 3, device=dev) * 2 - 1) * 0.55).contiguous()     # inside the volume (the border rule: test_gpu_field_query_grad)
    w = torch.randn(B, n, 4, device=dev)

    cfg = L.Cfg()
    cfg.B, cfg.V, cfg.C, cfg.H, cfg.L = B, V, Cc, H, len(spec.layers)
    for i, k in enumerate(spec.layers):
        cfg.layer_kind[i] = L.LAYER_CODE[k]
    cfg.voxel_length = 1.2
    cfg.flags = L.F_SIGMOID_RGB if spec.sigmoid_rgb else 0
    cfg.n_levels = len(lv)
    for i, (c, e) in enumerate(lv):
        cfg.level_V[i], cfg.level_C[i] = e, c
    cfg.precision = L.PREC_CODE[fwd]

    fp, gp = L.FieldParams(), L.FieldParamGrads()
    grads = {}

    def bind(slot_w, slot_b, i, key):
        for slot, suffix in ((slot_w, "weight"), (slot_b, "bias")):
            k = f"{key}.{suffix}"
            grads[k] = torch.zeros_like(prm[k])
            if i is None:
                setattr(fp, slot, prm[k].data_ptr())
                setattr(gp, slot, grads[k].data_ptr())
            else:
                getattr(fp, slot)[i] = prm[k].data_ptr()
                getattr(gp, slot)[i] = grads[k].data_ptr()

    for i, k in enumerate(spec.layers):
        bind("w", "b", i, f"network.{i}.layer")
    bind("w_final", "b_final", None, "final_layer")
    if variant == "TALLSIREN":
        bind("map_w1", "map_b1", None, "mapping_network.network.0")
        bind("map_w2", "map_b2", None, "mapping_network.network.2")
    n_film = spec.n_film
    if n_film:
        fo = torch.nn.functional.linear(glob, prm["mapping_network.weight"], prm["mapping_network.bias"])
        freq, phase = (fo[:, :n_film * H] * 15 + 30).contiguous(), fo[:, n_film * H:].contiguous()
    else:
        freq = phase = None

    levels, gl_levels = [], []
    vs, gvs = L.Volumes(), L.Volumes()
    for i, ((c, e), v) in enumerate(zip(lv, vols)):
        cl = torch.empty((B, e, e, e, c), device=dev)
        ok(lib.cnerf_fvol_channel_last(B, c, e, dptr(v), dptr(cl), stream), "channel_last")
        levels.append(cl)
        gl_levels.append(torch.zeros_like(cl))
        vs.level[i], gvs.level[i] = cl.data_ptr(), gl_levels[-1].data_ptr()

    a = C.c_size_t()
    ok(lib.cnerf_workspace_bytes(C.byref(cfg), C.byref(a), None, None), "workspace_bytes")
    packed = torch.empty(a.value // 4, device=dev)
    ok(lib.cnerf_pack_field(C.byref(cfg), C.byref(fp), dptr(packed), stream), "pack_field")
    out = torch.empty((B, n, 4), device=dev)
    ok(lib.cnerf_field_forward(C.byref(cfg), C.byref(vs), dptr(packed), p_or_null(freq), p_or_null(phase), dptr(pts), n, dptr(out), stream), "field_forward")

    nb = C.c_size_t()
    if bwd == "fp16":
        ok(lib.cnerf_backward16_bytes(C.byref(cfg), C.byref(nb)), "backward16_bytes")
        packed_bwd = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        ok(lib.cnerf_pack_field_chain16(C.byref(cfg), C.byref(fp), dptr(packed_bwd), stream), "pack_field_chain16")
    else:
        ok(lib.cnerf_backward_bytes(C.byref(cfg), C.byref(nb)), "backward_bytes")
        packed_bwd = torch.empty(nb.value, dtype=torch.uint8, device=dev)
        ok(lib.cnerf_pack_field_transposed(C.byref(cfg), C.byref(fp), dptr(packed_bwd), stream), "pack_field_transposed")
    bcode = L.PREC_CODE[bwd]
    ok(lib.cnerf_field_query_backward_workspace_bytes(C.byref(cfg), bcode, ppc, C.byref(nb)), "query_workspace_bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    g_freq = torch.zeros_like(freq) if n_film else None
    g_phase = torch.zeros_like(phase) if n_film else None
    g_pts = torch.zeros_like(pts)
    sat = torch.zeros(1, dtype=torch.int32, device=dev)
    ok(lib.cnerf_field_query_backward(C.byref(cfg), bcode, ppc, C.byref(vs), C.byref(fp), dptr(packed), dptr(packed_bwd), p_or_null(freq),
                                      p_or_null(phase), dptr(pts), n, dptr(out), dptr(w), C.byref(gp), p_or_null(g_freq), p_or_null(g_phase),
                                      C.byref(gvs), dptr(g_pts), dptr(sat), dptr(ws), stream), "field_query_backward")
    torch.cuda.synchronize()
    assert int(sat.item()) == 0

    # ---- against autograd through the oracle ----------------------------------------------------------------------------------------
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in prm.items()}
    vr = [v.detach().cpu().clone().requires_grad_(True) for v in vols]
    gr = glob.detach().cpu().clone().requires_grad_(True) if glob is not None else None
    pr = pts.detach().cpu().clone().requires_grad_(True)
    ref, _ = O.field_eval(spec, params, vr if len(vr) > 1 else vr[0], gr, pr)
    assert scaled_err(out.cpu().numpy(), ref.detach().numpy()) < 2e-4
    (ref * w.cpu()).sum().backward()

    def close(got, want, k):
        got, want = got.detach().cpu().double().numpy(), want.detach().double().numpy()
        rel_l2 = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
        print(f"{k:40s} rel l2 {rel_l2:.2e} scaled {scaled_err(got, want):.2e}")
        assert rel_l2 < (3e-3 if bwd == "fp16" else 2e-3), (k, rel_l2)
        assert scaled_err(got, want) < (5e-2 if bwd == "fp16" else 2e-2), (k, scaled_err(got, want))

    for k, g in grads.items():
        close(g, params[k].grad, k)
    for i, ((c, e), gl) in enumerate(zip(lv, gl_levels)):
        cf = torch.empty((B, c, e, e, e), device=dev)
        ok(lib.cnerf_fvol_channel_first(B, c, e, dptr(gl), dptr(cf), stream), "channel_first")
        close(cf, vr[i].grad, f"volume{i}")
    close(g_pts, pr.grad, "points")
    if n_film:           # the host finishes the mapping Linear: d fo = [15 dfreq | dphase]
        d_fo = torch.cat([15.0 * g_freq, g_phase], -1)
        close(d_fo.t() @ glob, params["mapping_network.weight"].grad, "mapping_network.weight")
        close(d_fo @ prm["mapping_network.weight"], gr.grad, "global_feature")
