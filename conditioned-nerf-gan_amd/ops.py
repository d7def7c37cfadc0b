"""Thin PyTorch-side wrappers over the C ABI (include/cnerf.h).  PyTorch only provides device memory, the current
stream and autograd plumbing here; every computation below happens in libcnerf_hip.so."""
import ctypes as C
import weakref
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import _lib as L

# packed weights per field network and layout: dropped with the module (weak keys), re-packed when a parameter's version changes
_pack_cache = weakref.WeakKeyDictionary()


def clear_pack_cache():
    """Forget every packed weight buffer (a training step that changed the weights re-packs anyway: the cache keys hold the
    parameters' version counters; bench.py calls this so that every timed step pays the packing like a training step)."""
    _pack_cache.clear()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def as_levels(vols):
    """Channel-last volume(s) -> list of (B,V,V,V,C) tensors."""
    return list(vols) if isinstance(vols, (list, tuple)) else [vols]


def volumes_struct(levels):
    v = L.Volumes()
    for i, t in enumerate(levels):
        L.ptr(t)
        v.level[i] = t.data_ptr()
    return v


def precision_of(net):
    """Forward arithmetic of `net`: its `.precision` attribute -- "fp32" (exact fp32 MFMA), "fp16x3" (fp32-accurate three-way
    fp16 split, same parity gate) or "fp16" (plain fp16 products with fp32 sums: the reference's autocast class, ~1e-3) -- the
    every layer family has the three kernels (FiLM / plain-sine / residual: field_h3.hip, per-point FiLM: field_pw16.hip)."""
    p = getattr(net, "precision", "fp32")
    if p not in L.PREC_CODE:
        raise L.CnerfError(f"unknown precision {p!r}")
    return p


def make_cfg(net, B, vols, R=1, S=2, fov=30.0, ray_start=0.0, ray_end=1.0, noise_std=0.0, hierarchical=False,
             white_back=False, last_back=False, clamp_mode="relu", precision=None, philox=None, drop=None):
    """cnerf_cfg for a field network `net` (generators.siren.FieldNetwork); vols: channel-last volume(s) or, for calls
    that touch no volume, the side V of a single 32-channel one; a network without a volume (SHORTSIREN) takes an empty list."""
    cfg = L.Cfg()
    no_volume = net.spec.input == "position"      # layer 0 reads the sample position and nothing else: CNERF_F_NO_VOLUME
    if no_volume:
        if not isinstance(vols, int) and len(as_levels(vols)):
            raise L.CnerfError(f"{net.variant} reads no feature volume")
        shapes = []
    elif isinstance(vols, int):
        shapes = [(vols, 32)]
    else:
        shapes = [(int(t.shape[1]), int(t.shape[-1])) for t in as_levels(vols)]
    if len(shapes) > L.MAX_LEVELS:
        raise L.CnerfError(f"at most {L.MAX_LEVELS} feature volumes")
    cfg.B, cfg.R, cfg.S, cfg.V = int(B), int(R), int(S), shapes[0][0] if shapes else 0
    cfg.C, cfg.H = sum(c for _, c in shapes), int(net.hidden_dim)
    cfg.n_levels = len(shapes)
    for i, (v, c) in enumerate(shapes):
        cfg.level_V[i], cfg.level_C[i] = v, c
    k0 = 3 if net.spec.input in ("xyz", "position") else cfg.C + (3 if net.spec.input == "feat_xyz" else 0)
    if not isinstance(vols, int) and k0 != int(net.input_dim):
        raise L.CnerfError(f"{net.variant}: layer 0 expects {net.input_dim} inputs, the feature volumes provide {k0}")
    kinds = [L.LAYER_CODE[k] for k in net.spec.layers]
    cfg.L = len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.ray_start, cfg.ray_end, cfg.voxel_length = float(ray_start), float(ray_end), 1.2
    cfg.noise_std = float(noise_std)
    cfg.fov_deg = float(fov)
    flags = _ray_flags(clamp_mode, white_back, last_back)
    flags |= L.F_HIERARCHICAL if hierarchical else 0
    flags |= L.F_SIGMOID_RGB if net.spec.sigmoid_rgb else 0
    flags |= L.F_INPUT_XYZ if net.spec.input == "feat_xyz" else 0
    flags |= L.F_NO_VOLUME if no_volume else 0
    cfg.flags = flags
    cfg.precision = L.PREC_CODE[precision if precision is not None else precision_of(net)]
    if philox is not None:            # (seed, offset): draws without a tensor are generated in the kernels
        cfg.philox, cfg.philox_seed, cfg.philox_offset = 1, int(philox[0]) & 0xFFFFFFFFFFFFFFFF, int(philox[1]) & 0xFFFFFFFF
    if drop is not None:              # (p, (seed, offset)): dropout of a network in training mode, see drop_of()
        cfg.drop_p = float(drop[0])
        if philox is None:            # the key of the keep decisions (the four draws stay tensors: cfg.philox = 0)
            cfg.philox_seed, cfg.philox_offset = int(drop[1][0]) & 0xFFFFFFFFFFFFFFFF, int(drop[1][1]) & 0xFFFFFFFF
    return cfg


def _ray_flags(clamp_mode, white_back, last_back):
    """cnerf_cfg.flags of the compositing: clamp mode, white / last background."""
    if clamp_mode not in ("relu", "softplus"):
        raise TypeError("Need to choose clamp mode")   # the reference raises a str here, i.e. a TypeError
    return (L.F_WHITE_BACK if white_back else 0) | (L.F_LAST_BACK if last_back else 0) | (L.F_SOFTPLUS if clamp_mode == "softplus" else 0)


def drop_of(rng):
    """rng["drop"] = (p, (seed, offset)) when the network drops out in this call (ImplicitGenerator3d.forward sets it in training mode)."""
    return (rng or {}).get("drop")


def _float3(v):
    """Three floats for a `const float[3]` argument; a number stands for all three."""
    v = (v, v, v) if isinstance(v, (int, float)) else tuple(v)
    return (C.c_float * 3)(*(float(x) for x in v))


def _workspace(entry_name, dev, *dims):
    """The workspace that the size query `entry_name` asks for at `dims`: uint8 on `dev`, or None where it asks for nothing."""
    nb = C.c_size_t(0)
    L.check(getattr(L.lib(), entry_name)(*dims, C.byref(nb)), entry_name)
    return torch.empty(nb.value, dtype=torch.uint8, device=dev) if nb.value else None


def _u8(t):
    return None if t is None else t.to(torch.uint8).contiguous()


def sizes(cfg, render=True):
    a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    L.check(L.lib().cnerf_workspace_bytes(C.byref(cfg), C.byref(a), C.byref(b), C.byref(c) if render else None),
            "cnerf_workspace_bytes")
    return a.value, b.value, c.value


def _params_struct(struct, net, tensors):
    """cnerf_field_params (struct = L.FieldParams) or cnerf_field_param_grads (L.FieldParamGrads) over a flat tensor list in the order
    of net.field_params() (mapping MLP first for the per-point family)."""
    fp = struct()
    it = iter(tensors)
    if net.spec.input == "xyz":
        fp.map_w1, fp.map_b1, fp.map_w2, fp.map_b2 = (next(it).data_ptr() for _ in range(4))
    for i, kind in enumerate(net.spec.layers):
        fp.w[i], fp.b[i] = next(it).data_ptr(), next(it).data_ptr()
        if kind == "res":
            fp.w2[i], fp.b2[i] = next(it).data_ptr(), next(it).data_ptr()
    fp.w_final, fp.b_final = next(it).data_ptr(), next(it).data_ptr()
    return fp


def _cached_pack(net, cfg, layout, nbytes, entry, dtype):
    """The buffer the ABI entry point `entry` (cfg, field params, buffer, stream) packs from the parameters of `net`, cached per
    (net, layout) and re-packed only when a parameter changed; nbytes() sizes it on a miss."""
    key = tuple((p.data_ptr(), p._version) for p in net.field_params())
    hit = _pack_cache.setdefault(net, {}).get(layout)
    if hit is not None and hit[0] == key:
        return hit[1]
    params = [_f32(p.detach()) for p in net.field_params()]
    buf = torch.empty(nbytes() // dtype.itemsize, dtype=dtype, device=params[0].device)
    fp = _params_struct(L.FieldParams, net, params)
    L.check(getattr(L.lib(), entry)(C.byref(cfg), C.byref(fp), L.ptr(buf), _stream()), entry)
    buf._keepalive = params
    _pack_cache[net][layout] = (key, buf)
    return buf


def _abi_bytes(entry, cfg):
    nb = C.c_size_t(0)
    L.check(getattr(L.lib(), entry)(C.byref(cfg), C.byref(nb)), entry)
    return nb.value


def pack_field(net, cfg):
    """Packed MFMA-order weights of `net` in cfg's precision (cnerf_pack_field)."""
    return _cached_pack(net, cfg, ("forward", cfg.precision), lambda: sizes(cfg, render=False)[0], "cnerf_pack_field", torch.float32)


def channel_last_levels(vols):
    """Channel-first volume or list of volumes -> list of channel-last volumes."""
    return [channel_last(v) for v in as_levels(vols)]


def channel_last(fvol):
    """(B,C,V,V,V) -> (B,V,V,V,C) on the GPU (C a multiple of 32).  A volume that already lives in memory channel-last
    (torch.channels_last_3d, e.g. an encoder whose last convolution writes that format: SURVEY.md 8f-1) is taken as it is:
    no transpose kernel, no copy."""
    if fvol.dim() == 5 and fvol.dtype == torch.float32 and fvol.is_cuda:
        view = fvol.detach().permute(0, 2, 3, 4, 1)
        if view.is_contiguous() and fvol.shape[2] == fvol.shape[3] == fvol.shape[4]:
            return view
    fvol = _f32(fvol)
    B, Cc, V = fvol.shape[0], fvol.shape[1], fvol.shape[-1]
    if fvol.shape[2:] != (V, V, V):
        raise L.CnerfError("feature volume must be cubic (B,C,V,V,V)")
    out = torch.empty((B, V, V, V, Cc), dtype=torch.float32, device=fvol.device)
    L.check(L.lib().cnerf_fvol_channel_last(B, Cc, V, L.ptr(fvol), L.ptr(out), _stream()), "cnerf_fvol_channel_last")
    return out


def channel_first(fvol_cl):
    fvol_cl = _f32(fvol_cl)
    B, V, Cc = fvol_cl.shape[0], fvol_cl.shape[1], fvol_cl.shape[-1]
    out = torch.empty((B, Cc, V, V, V), dtype=torch.float32, device=fvol_cl.device)
    L.check(L.lib().cnerf_fvol_channel_first(B, Cc, V, L.ptr(fvol_cl), L.ptr(out), _stream()), "cnerf_fvol_channel_first")
    return out


def gather_features(net, fvol_cl, points):
    points = _f32(points)
    B, n = points.shape[0], points.shape[1]
    cfg = make_cfg(net, B, int(fvol_cl.shape[1]))
    out = torch.empty((B, n, fvol_cl.shape[-1]), dtype=torch.float32, device=points.device)
    L.check(L.lib().cnerf_gather_features(C.byref(cfg), L.ptr(fvol_cl), L.ptr(points), n, L.ptr(out), _stream()),
            "cnerf_gather_features")
    return out


def field_forward(net, fvol, freq, phase, points, fvol_is_channel_last=False, drop=None):
    """rgb_sigma (B,n,4) of `net` at explicit world points (B,n,3).  drop = (p, (seed, offset)): dropout of a training-mode call.
    Differentiable (FieldQueryFunction) w.r.t. the volume(s), freq / phase, the points and the field parameters when grad mode is
    on and one of them requires grad; otherwise the plain forward without an autograd node."""
    vols = as_levels(fvol)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (freq, phase, points, *vols, *net.field_params())):
        return FieldQueryFunction.apply(net, drop, bool(fvol_is_channel_last), freq, phase, points, len(vols), *vols, *net.field_params())
    return _field_forward(net, fvol, freq, phase, points, fvol_is_channel_last, drop)


def _field_forward(net, fvol, freq, phase, points, fvol_is_channel_last=False, drop=None):
    points = _f32(points)
    B, n = points.shape[0], points.shape[1]
    levels = [_f32(v) for v in as_levels(fvol)] if fvol_is_channel_last else channel_last_levels(fvol)
    cfg = make_cfg(net, B, levels, drop=drop)
    packed = pack_field(net, cfg)
    out = torch.empty((B, n, 4), dtype=torch.float32, device=points.device)
    vs = volumes_struct(levels)
    L.check(L.lib().cnerf_field_forward(C.byref(cfg), C.byref(vs), L.ptr(packed), L.ptr(_f32(freq)), L.ptr(_f32(phase)),
                                        L.ptr(points), n, L.ptr(out), _stream()), "cnerf_field_forward")
    return out


def composite(rgb_sigma, z, eps=None, noise_std=0.0, clamp_mode="relu", white_back=False, last_back=False):
    """fancy_integration on (rays,n,4)/(rays,n) tensors -> rgb (rays,3), dist (rays), weights (rays,n)."""
    rgb_sigma, z, eps = _f32(rgb_sigma), _f32(z), _f32(eps)
    rays, n = z.shape
    cfg = L.Cfg()
    cfg.noise_std = float(noise_std)
    cfg.flags = _ray_flags(clamp_mode, white_back, last_back)
    dev = z.device
    rgb = torch.empty((rays, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((rays,), dtype=torch.float32, device=dev)
    w = torch.empty((rays, n), dtype=torch.float32, device=dev)
    L.check(L.lib().cnerf_composite(C.byref(cfg), rays, n, L.ptr(rgb_sigma), L.ptr(z), L.ptr(eps), L.ptr(rgb), L.ptr(dist),
                                    L.ptr(w), _stream()), "cnerf_composite")
    return rgb, dist, w


def resample(z, weights, u):
    """Inverse-CDF depths: z, weights, u (rays,S) -> fine_z (rays,S), inds (rays,S) int32, cdf (rays,S-1)."""
    z, weights, u = _f32(z), _f32(weights), _f32(u)
    rays, S = z.shape
    dev = z.device
    fine = torch.empty((rays, S), dtype=torch.float32, device=dev)
    inds = torch.empty((rays, S), dtype=torch.int32, device=dev)
    cdf = torch.empty((rays, S - 1), dtype=torch.float32, device=dev)
    L.check(L.lib().cnerf_resample(rays, S, L.ptr(z), L.ptr(weights), L.ptr(u), L.ptr(fine), L.ptr(inds), L.ptr(cdf),
                                   _stream()), "cnerf_resample")
    return fine, inds, cdf


def philox_fill(seed, offset, stream_id, n, normal, device):
    """The draws the kernels generate under cnerf_cfg.philox, as a tensor: stream 0 u_strat, 1 eps_coarse, 2 u_fine, 3 eps_final."""
    out = torch.empty(int(n), dtype=torch.float32, device=device)
    L.check(L.lib().cnerf_philox_fill(int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFF, int(stream_id), int(n), 1 if normal else 0,
                                      L.ptr(out), _stream()), "cnerf_philox_fill")
    return out


def _rng_struct(rng, keys):
    """(cnerf_rng, the tensors behind it) of the draws `keys` in rng: float32, the injected dropout decisions (tests) uint8."""
    r, keep = L.Rng(), []
    for k in keys:
        t = (_u8 if k.startswith("drop_") else _f32)(rng.get(k))
        L.ptr(t)   # validates device / contiguity
        setattr(r, k, None if t is None else t.data_ptr())
        keep.append(t)
    return r, keep


def _act16_aux(act16, aux=None):
    """`aux` (or a new cnerf_aux) carrying the fp16 activations of the field passes: one (feat, h, c[, amax]) set per pass."""
    aux = aux if aux is not None else L.Aux()
    for i, bufs in enumerate(act16):
        aux.act16[i].feat, aux.act16[i].h, aux.act16[i].c = (t.data_ptr() for t in bufs[:3])
        if len(bufs) > 3:
            aux.act16[i].amax = bufs[3].data_ptr()
    return aux


AUX_SHAPES = {
    "coarse_points": lambda B, P, S, n: ((B, P, S, 3), torch.float32),
    "coarse_z": lambda B, P, S, n: ((B, P, S), torch.float32),
    "coarse_rgb_sigma": lambda B, P, S, n: ((B, P, S, 4), torch.float32),
    "coarse_weights": lambda B, P, S, n: ((B, P, S), torch.float32),
    "cdf": lambda B, P, S, n: ((B, P, S - 1), torch.float32),
    "inds": lambda B, P, S, n: ((B, P, S), torch.int32),
    "fine_z": lambda B, P, S, n: ((B, P, S), torch.float32),
    "fine_rgb_sigma": lambda B, P, S, n: ((B, P, S, 4), torch.float32),
    "sort_idx": lambda B, P, S, n: ((B, P, 2 * S), torch.int32),
    "final_weights": lambda B, P, S, n: ((B, P, n), torch.float32),
    "fine_points": lambda B, P, S, n: ((B, P, S, 3), torch.float32),
}
HIER_ONLY = {"coarse_weights", "cdf", "inds", "fine_z", "fine_rgb_sigma", "sort_idx", "fine_points"}


def _aux_buffers(want_aux, aux_keys, B, P, S, n, hier, dev):
    """({key: tensor}, the cnerf_aux pointing at them or None) of the intermediates a render keeps: all of L.AUX_FIELDS (want_aux) or
    aux_keys, without the hierarchical-only ones where there is no fine pass."""
    aux_t, aux_s = {}, None
    if want_aux or aux_keys:
        aux_s = L.Aux()
        for k in (L.AUX_FIELDS if want_aux else aux_keys):
            if not hier and k in HIER_ONLY:
                continue
            shape, dt = AUX_SHAPES[k](B, P, S, n)
            aux_t[k] = torch.empty(shape, dtype=dt, device=dev)
            setattr(aux_s, k, aux_t[k].data_ptr())
    return aux_t, aux_s


def render_forward(net, fvol, freq, phase, cam2world, img_size, fov, ray_start, ray_end, num_steps, hierarchical,
                   clamp_mode, noise_std, white_back=False, last_back=False, rng: Optional[dict] = None,
                   want_aux=False, fvol_is_channel_last=False, field_events=None, aux_keys=None, act16=None):
    """ImplicitGenerator3d.forward on the GPU.  rng: dict with u_strat / eps_coarse / u_fine / eps_final tensors.
    field_events: optional 4 hipEvent_t handles (ints) recorded around the two field-kernel launches."""
    cam2world = _f32(cam2world)
    B, R, S = cam2world.shape[0], int(img_size), int(num_steps)
    P = R * R
    n = 2 * S if hierarchical else S
    dev = cam2world.device
    levels = [_f32(v) for v in as_levels(fvol)] if fvol_is_channel_last else channel_last_levels(fvol)
    cfg = make_cfg(net, B, levels, R, S, fov, ray_start, ray_end, noise_std, hierarchical, white_back,
                   last_back, clamp_mode, philox=(rng or {}).get("philox"), drop=drop_of(rng))
    vs = volumes_struct(levels)
    packed = pack_field(net, cfg)
    _, _, ws_bytes = sizes(cfg)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pixels = torch.empty((B, 3, R, R), dtype=torch.float32, device=dev)
    depth = torch.empty((B, R, R), dtype=torch.float32, device=dev)
    r, keep = _rng_struct(rng or {}, ("u_strat", "eps_coarse", "u_fine", "eps_final", "fine_z", "drop_coarse", "drop_fine"))
    aux_t, aux_s = _aux_buffers(want_aux, aux_keys, B, P, S, n, hierarchical, dev)
    if field_events is not None:
        aux_s = aux_s if aux_s is not None else L.Aux()
        for i, ev in enumerate(field_events):
            aux_s.field_events[i] = ev
    if act16 is not None:          # keep the field passes' activations (fp16 tile blocks) for the half-precision backward
        aux_s = _act16_aux(act16, aux_s)
    L.check(L.lib().cnerf_render_forward(C.byref(cfg), C.byref(vs), L.ptr(packed), L.ptr(_f32(freq)), L.ptr(_f32(phase)),
                                         L.ptr(cam2world), C.byref(r), L.ptr(pixels), L.ptr(depth),
                                         C.byref(aux_s) if aux_s is not None else None, L.ptr(ws), _stream()),
            "cnerf_render_forward")
    return pixels, depth, aux_t


# ---------------------------------------------------------------------------------------------------------------------
# autograd
# ---------------------------------------------------------------------------------------------------------------------
SAVED_KEYS = ("coarse_rgb_sigma", "coarse_z", "fine_rgb_sigma", "fine_z")


def pack_field_transposed(net, cfg):
    """Transposed fp32 weights of the exact gradient chain (cnerf_pack_field_transposed)."""
    return _cached_pack(net, cfg, "transposed", lambda: _abi_bytes("cnerf_backward_bytes", cfg), "cnerf_pack_field_transposed", torch.float32)


PHASE_TIMER = None              # an object with begin() / end(name, start) (training.gan_step.PhaseTimer): RenderFunction.backward
                                # reports its span as "render_bwd" so that a caller can split an autograd pass (bench.py gan_step)
ACT_BUDGET_BYTES = 128 << 30    # chunk buffers of the per-point FiLM family's fp32 backward: at most this much, and MEMORY_FRACTION of what is free


def backward_precision_of(net):
    """Arithmetic of the backward's gradient GEMMs: `net.backward_precision` = "fp32" (exact fp32 MFMA chain and weight
    gradients, the default) or "fp16" (fp16 operands, fp32 sums: the reference's own training numerics, utils.py:643 autocast):
    bwd16.hip for FiLM / plain-sine / residual-block networks, chain_pw16.hip for the per-point FiLM family."""
    p = getattr(net, "backward_precision", "fp32")
    if p not in ("fp32", "fp16"):
        raise L.CnerfError(f"unknown backward precision {p!r}")
    return p


def n_matrices(net):
    """Weight matrices before the head ("slabs" of the backward's buffers): a residual block has two."""
    return sum(2 if k == "res" else 1 for k in net.spec.layers)


def pack_field_chain16(net, cfg):
    """Transposed fp16 weight units of the half-precision gradient chain (cnerf_pack_field_chain16)."""
    return _cached_pack(net, cfg, "chain16", lambda: _abi_bytes("cnerf_backward16_bytes", cfg), "cnerf_pack_field_chain16", torch.uint8)


RESIDENT_BUDGET_BYTES = 160 << 30    # fp16 activations kept from the forward for the backward: at most this much (288 GB of HBM per GPU) ...
RESIDENT_FRACTION = 0.5              # ... and at most this share of the memory that is free when the forward starts


def resident_act16(net, levels, B, R, S, hier, dev):
    """fp16 tile-block buffers that keep the activations of the forward's field passes for the half-precision backward (one
    set per pass: x0, sin, cos), or None when they would not fit the budget -- the backward then re-computes them chunk-wise."""
    H, NT = int(net.hidden_dim), int(net.hidden_dim) // 32
    n_in = sum(int(t.shape[-1]) for t in levels) // 32 + (1 if net.spec.input in ("feat_xyz", "position") else 0)
    nslab = n_matrices(net)
    T = B * ((R * R * S + 31) // 32)
    n_pass = 2 if hier else 1
    f16 = dict(dtype=torch.float16, device=dev)
    if net.spec.layers[0] == "pfilm":      # field_pw16.hip: feature + position | y_l slabs then m | cos, cos f, cos 15 pre per layer | per-point maxima
        blocks = 2 + nslab * NT + 8 + 3 * nslab * NT
        if n_pass * T * 2048 * blocks + T * 2048 * (3 * nslab * NT + 9) > min(RESIDENT_BUDGET_BYTES, RESIDENT_FRACTION * free_device_bytes(dev)):
            return None
        return [(torch.empty((T, 2, 32, 32), **f16), torch.empty(((nslab * NT + 8) * T, 32, 32), **f16), torch.empty((3 * nslab, T, NT, 32, 32), **f16),
                 torch.empty((nslab, T * 32), dtype=torch.float32, device=dev)) for _ in range(n_pass)]
    per_pass = T * 2048 * (n_in + 2 * nslab * NT)
    if n_pass * per_pass + T * 2048 * (nslab * NT + 1) > min(RESIDENT_BUDGET_BYTES, RESIDENT_FRACTION * free_device_bytes(dev)):
        return None
    return [(torch.empty((T, n_in, 32, 32), **f16), torch.empty((nslab, T, NT, 32, 32), **f16), torch.empty((nslab, T, NT, 32, 32), **f16))
            for _ in range(n_pass)]


def free_device_bytes(dev):
    """What an allocation could get right now: the driver's free memory plus what torch's caching allocator holds unused."""
    free, _ = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)


def backward_chunk(cfg, bprec_code, B, have_act16, dev):
    """(images per chunk, workspace bytes) of cnerf_render_backward: the largest chunk whose workspace fits MEMORY_FRACTION of the
    memory that is free NOW -- not a constant sized for an empty 288 GB part: whatever the encoder, the discriminator
    and DDP already hold is accounted for, and a smaller or shared device gets smaller chunks instead of an out-of-memory error.
    The per-point FiLM family's fp32 backward takes ACT_BUDGET_BYTES at most."""
    budget = int(MEMORY_FRACTION * free_device_bytes(dev))
    if cfg.layer_kind[0] == L.LAYER_PFILM and bprec_code == L.PREC_FP32:
        budget = min(budget, ACT_BUDGET_BYTES)
    need = C.c_size_t(0)
    for nb in ([B] if have_act16 else range(B, 0, -1)):
        L.check(L.lib().cnerf_backward_workspace_bytes(C.byref(cfg), bprec_code, nb, 1 if have_act16 else 0, C.byref(need)), "cnerf_backward_workspace_bytes")
        if need.value <= budget or nb == 1:
            break
    if need.value > budget:
        raise L.CnerfError(f"render backward: one image needs {need.value / 2**30:.1f} GiB of chunk buffers, {budget / 2**30:.1f} GiB are free")
    return nb, need.value


MEMORY_FRACTION = 0.8
LAST_SATURATED = None          # device int32 tensor of the most recent fp16 backward: clamped (tile, matrix) blocks, see include/cnerf.h


def _backward_setup(net, cfg, levels, B, dev):
    """What render_backward and query_backward hand to the library besides their own inputs: the packed weights of the re-run (cfg's
    precision) and of the gradient chain (fp16 units, or the transposed fp32 weights), the field parameters, zeroed gradients of the
    parameters, of freq / phase (FiLM layers) and of the volume levels, their structs, and the fp16 backward's saturation counter."""
    bprec = backward_precision_of(net)
    packed = pack_field(net, cfg)
    packed_bwd = pack_field_chain16(net, cfg) if bprec == "fp16" else pack_field_transposed(net, make_cfg(net, B, levels, precision="fp32"))
    params = [_f32(p.detach()) for p in net.field_params()]
    grads = [torch.zeros_like(p) for p in params]
    n_film = sum(1 for k in net.spec.layers if k == "film")
    g_freq = torch.zeros((B, n_film * int(net.hidden_dim)), dtype=torch.float32, device=dev) if n_film else None
    grad_levels = [torch.zeros_like(v) for v in levels]
    return SimpleNamespace(code=L.PREC_CODE[bprec], packed=packed, packed_bwd=packed_bwd, params=params, grads=grads,
                           fp=_params_struct(L.FieldParams, net, params), gp=_params_struct(L.FieldParamGrads, net, grads),
                           g_freq=g_freq, g_phase=torch.zeros_like(g_freq) if n_film else None, grad_levels=grad_levels,
                           vs=volumes_struct(levels), gvs=volumes_struct(grad_levels),
                           sat=torch.zeros(1, dtype=torch.int32, device=dev) if bprec == "fp16" else None)


def merge_composite_backward(cfg, coarse_rgb_sigma, coarse_z, fine_rgb_sigma, fine_z, eps_final, grad_pixels, grad_depth):
    """Step 1 of the backward on its own (cnerf_merge_composite_backward): d loss / d pixels (B,3,R,R) and d loss / d depth (B,R,R), or
    None -> d loss / d rgb_sigma of the coarse and of the fine samples, each (B,P,S,4); the fine one is None when cfg is not hierarchical
    (the fine tensors are then ignored).  eps_final (B,P,n): the injected density noise of the final composite, None for none."""
    hier = bool(cfg.flags & L.F_HIERARCHICAL)
    c_rs, c_z, grad_pixels = _f32(coarse_rgb_sigma), _f32(coarse_z), _f32(grad_pixels)
    f_rs, f_z = (_f32(fine_rgb_sigma), _f32(fine_z)) if hier else (None, None)
    eps_final, grad_depth = _f32(eps_final), _f32(grad_depth)
    gc = torch.empty_like(c_rs)
    gf = torch.empty_like(f_rs) if hier else None
    L.check(L.lib().cnerf_merge_composite_backward(C.byref(cfg), L.ptr(c_rs), L.ptr(c_z), L.ptr(f_rs), L.ptr(f_z), L.ptr(eps_final),
                                                   L.ptr(grad_pixels), L.ptr(grad_depth), L.ptr(gc), L.ptr(gf), _stream()),
            "cnerf_merge_composite_backward")
    return gc, gf


def render_backward(net, o, levels, freq, phase, cam2world, rng, saved, grad_pixels, grad_depth, act16=None):
    """Gradients of one render w.r.t. (channel-last feature volumes, freq, phase, [field parameters]): ONE call into the library
    (cnerf_render_backward)."""
    global LAST_SATURATED
    B, R, S, hier = o["B"], o["R"], o["S"], o["hier"]
    dev = cam2world.device
    bprec = backward_precision_of(net)
    pfilm32 = net.spec.layers[0] == "pfilm" and bprec == "fp32"
    # cfg: precision of the forward (the activation-storing re-run follows it); the fp16 backward re-runs the fp16x3 kernel, the per-point
    # FiLM family's fp32 chain the fp32 kernel (its packed weights are that kernel's)
    cfg = make_cfg(net, B, levels, R, S, o["fov"], o["ray_start"], o["ray_end"], o["noise_std"], hier, o["white_back"], o["last_back"],
                   o["clamp_mode"], precision="fp16x3" if bprec == "fp16" else ("fp32" if pfilm32 else None), philox=rng.get("philox"),
                   drop=drop_of(rng))
    c_rs, c_z, f_rs, f_z = saved[:4]
    grad_pixels = _f32(grad_pixels)
    grad_depth = _f32(grad_depth) if grad_depth is not None else None
    w = _backward_setup(net, cfg, levels, B, dev)
    nb, ws_bytes = backward_chunk(cfg, w.code, B, act16 is not None, dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    r, keep = _rng_struct(rng, ("u_strat", "eps_final", "drop_coarse", "drop_fine"))
    sv = L.Saved()
    sv.coarse_rgb_sigma, sv.coarse_z = c_rs.data_ptr(), c_z.data_ptr()
    if hier:
        sv.fine_rgb_sigma, sv.fine_z = f_rs.data_ptr(), f_z.data_ptr()
    for t in (c_rs, c_z) + ((f_rs, f_z) if hier else ()):
        L.ptr(t)
    aux = _act16_aux(act16) if act16 is not None else None
    L.check(L.lib().cnerf_render_backward(C.byref(cfg), w.code, nb, C.byref(w.vs), C.byref(w.fp), L.ptr(w.packed), L.ptr(w.packed_bwd), L.ptr(freq),
                                          L.ptr(phase), L.ptr(cam2world), C.byref(r), C.byref(sv), C.byref(aux) if aux is not None else None,
                                          L.ptr(grad_pixels), L.ptr(grad_depth), C.byref(w.gp), L.ptr(w.g_freq), L.ptr(w.g_phase), C.byref(w.gvs),
                                          L.ptr(w.sat), L.ptr(ws), _stream()), "cnerf_render_backward")
    if w.sat is not None:
        LAST_SATURATED = w.sat
    return w.grad_levels, w.g_freq, w.g_phase, w.grads


def _is_channel_last(levels, vols):
    """Per volume: did it arrive channels_last_3d, so that channel_last() took it as it is (zero-copy)?"""
    return [lv.data_ptr() == v.data_ptr() and not v.is_contiguous() for lv, v in zip(levels, vols)]


def _caller_format(g_levels, vol_is_cl):
    """Channel-last volume gradients in the memory format their volumes came in: a channels_last_3d volume gets a view, the others a
    channel-first copy."""
    return [g.permute(0, 4, 1, 2, 3) if cl else channel_first(g) for g, cl in zip(g_levels, vol_is_cl)]


class RenderFunction(torch.autograd.Function):
    """ImplicitGenerator3d.forward as one autograd node: differentiable w.r.t. the feature volume(s), freq/phase (and
    through them the mapping network and the global feature) and the field parameters; not w.r.t. cameras or sample
    positions (the reference runs those under no_grad: generators.py:57,111)."""

    @staticmethod
    def forward(ctx, net, o, rng, cam2world, freq, phase, n_vols, *rest):
        vols, params = rest[:n_vols], rest[n_vols:]
        levels = [channel_last(v.detach()) for v in vols]
        ctx.vol_is_cl = _is_channel_last(levels, vols)
        fr = freq.detach() if freq is not None else None
        ph = phase.detach() if phase is not None else None
        need_grad = o.get("need_grad", any(ctx.needs_input_grad))   # (decided by ops.render: grad mode is always off in here)
        act16 = None
        if need_grad and backward_precision_of(net) == "fp16" and precision_of(net) in (("fp16x3",) if net.spec.layers[0] == "pfilm" else ("fp16x3", "fp16")):
            act16 = resident_act16(net, levels, cam2world.shape[0], o["R"], o["S"], o["hier"], cam2world.device)
        pixels, depth, aux = render_forward(net, levels, fr, ph, cam2world, o["R"], o["fov"], o["ray_start"], o["ray_end"],
                                            o["S"], o["hier"], o["clamp_mode"], o["noise_std"], o["white_back"],
                                            o["last_back"], rng, want_aux=o["want_aux"], fvol_is_channel_last=True,
                                            field_events=o.get("field_events"),
                                            aux_keys=SAVED_KEYS if need_grad and not o["want_aux"] else None, act16=act16)
        ctx.net, ctx.o, ctx.rng, ctx.n_vols = net, o, rng, n_vols
        ctx.act16 = act16
        if need_grad:
            saved = [aux.get(k) for k in SAVED_KEYS]
            if o["hier"] and rng.get("fine_z") is not None:
                saved[3] = _f32(rng["fine_z"]).reshape(saved[1].shape)   # teacher-forced depths are what the fine pass used
            ctx.saved = (levels, fr, ph, _f32(cam2world), tuple(saved))
        RenderFunction.last_aux = aux
        return pixels, depth

    @staticmethod
    def backward(ctx, grad_pixels, grad_depth):
        levels, fr, ph, cam2world, saved = ctx.saved
        t0 = PHASE_TIMER.begin() if PHASE_TIMER is not None else None
        g_levels, g_freq, g_phase, g_params = render_backward(ctx.net, ctx.o, levels, fr, ph, cam2world, ctx.rng, saved,
                                                              grad_pixels.contiguous(),
                                                              grad_depth.contiguous() if grad_depth is not None else None,
                                                              act16=ctx.act16)
        ctx.act16 = None
        g_vols = _caller_format(g_levels, ctx.vol_is_cl)
        if t0 is not None:
            PHASE_TIMER.end("render_bwd", t0)
        return (None, None, None, None, g_freq, g_phase, None, *g_vols, *g_params)


def render(net, fvol, freq, phase, cam2world, img_size, fov, ray_start, ray_end, num_steps, hierarchical, clamp_mode,
           noise_std, white_back=False, last_back=False, rng=None, want_aux=False, field_events=None):
    """Differentiable entry used by ImplicitGenerator3d.forward.  fvol: (B,C,V,V,V) or a list of pyramid levels.
    Returns (pixels, depth, aux dict)."""
    o = dict(B=cam2world.shape[0], R=int(img_size), S=int(num_steps), fov=float(fov), ray_start=float(ray_start),
             ray_end=float(ray_end), hier=bool(hierarchical), clamp_mode=clamp_mode, noise_std=float(noise_std),
             white_back=bool(white_back), last_back=bool(last_back), want_aux=bool(want_aux), field_events=field_events)
    _ray_flags(clamp_mode, white_back, last_back)      # refuses an unknown clamp mode before any work
    vols = as_levels(fvol)
    # Will anything back-propagate through this render?  Decided HERE: inside Function.forward grad mode is always off, and
    # ctx.needs_input_grad is True for every parameter even under torch.no_grad() -- the D step's no-grad renders then ran the
    # activation-storing forward (14.7 instead of 9.9 ms per launch at batch 8) and allocated the kept activations for nothing.
    params = net.field_params()
    o["need_grad"] = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (freq, phase, *vols, *params))
    pixels, depth = RenderFunction.apply(net, o, rng or {}, cam2world, freq, phase, len(vols), *vols, *params)
    return pixels, depth, (RenderFunction.last_aux if want_aux else {})


# ---------------------------------------------------------------------------------------------------------------------
# autograd of a field query: <SIREN>.forward(points, z) (siren.py:628-670) as one node
# ---------------------------------------------------------------------------------------------------------------------
def query_chunk(n, bytes_of, dev):
    """(points per chunk, bytes) of a field query's backward: all n points when bytes_of(n) fits MEMORY_FRACTION of the memory that
    is free now, else the largest share of n -- halved until it fits, a multiple of 32 -- whose buffers do."""
    budget = int(MEMORY_FRACTION * free_device_bytes(dev))
    ppc = int(n)
    need = bytes_of(ppc)
    while need > budget and ppc > 32:
        ppc = max(32, (ppc // 2 + 31) // 32 * 32)
        need = bytes_of(ppc)
    if need > budget:
        raise L.CnerfError(f"field query backward: {ppc} points need {need / 2**30:.1f} GiB of chunk buffers, {budget / 2**30:.1f} GiB are free")
    return ppc, need


def query_workspace_bytes(cfg, bprec_code, points_per_chunk):
    nb = C.c_size_t(0)
    L.check(L.lib().cnerf_field_query_backward_workspace_bytes(C.byref(cfg), bprec_code, int(points_per_chunk), C.byref(nb)),
            "cnerf_field_query_backward_workspace_bytes")
    return nb.value


def query_backward(net, levels, freq, phase, points, out, grad_out, drop, want_points):
    """Gradients of one field query w.r.t. (channel-last volume levels, freq, phase, field parameters, points or None): ONE call into
    the library (cnerf_field_query_backward).  The backward precision and the re-run's precision follow render_backward."""
    global LAST_SATURATED
    B, n = points.shape[0], points.shape[1]
    dev = points.device
    bprec = backward_precision_of(net)
    g_pts = torch.zeros_like(points) if want_points else None
    pfilm32 = net.spec.layers[0] == "pfilm" and bprec == "fp32"
    cfg = make_cfg(net, B, levels, precision="fp16x3" if bprec == "fp16" else ("fp32" if pfilm32 else None), drop=drop)
    w = _backward_setup(net, cfg, levels, B, dev)
    ppc, ws_bytes = query_chunk(n, lambda k: query_workspace_bytes(cfg, w.code, k), dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    L.check(L.lib().cnerf_field_query_backward(C.byref(cfg), w.code, ppc, C.byref(w.vs), C.byref(w.fp), L.ptr(w.packed), L.ptr(w.packed_bwd),
                                               L.ptr(freq), L.ptr(phase), L.ptr(points), n, L.ptr(out), L.ptr(grad_out), C.byref(w.gp),
                                               L.ptr(w.g_freq), L.ptr(w.g_phase), C.byref(w.gvs), L.ptr(g_pts), L.ptr(w.sat), L.ptr(ws), _stream()),
            "cnerf_field_query_backward")
    if w.sat is not None:
        LAST_SATURATED = w.sat
    return w.grad_levels, w.g_freq, w.g_phase, w.grads, g_pts


class FieldQueryFunction(torch.autograd.Function):
    """<SIREN>.forward(points, z) as one autograd node: differentiable w.r.t. the feature volume(s), freq / phase (and through them the
    mapping network and the global feature), the query points and the field parameters.  drop = (p, (seed, offset)) of a training-mode
    call is kept for the backward, which draws the same keep decisions whatever its chunking."""

    @staticmethod
    def forward(ctx, net, drop, vols_channel_last, freq, phase, points, n_vols, *rest):
        vols, params = rest[:n_vols], rest[n_vols:]
        levels = [_f32(v.detach()) for v in vols] if vols_channel_last else [channel_last(v.detach()) for v in vols]
        # volumes given channel-last get channel-last gradients, the others their caller's format
        ctx.vols_channel_last = vols_channel_last
        ctx.vol_is_cl = _is_channel_last(levels, vols)
        fr = _f32(freq.detach()) if freq is not None else None
        ph = _f32(phase.detach()) if phase is not None else None
        pts = _f32(points.detach())
        out = _field_forward(net, levels, fr, ph, pts, fvol_is_channel_last=True, drop=drop)
        ctx.net, ctx.drop, ctx.n_vols = net, drop, n_vols
        ctx.saved = (levels, fr, ph, pts)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        levels, fr, ph, pts = ctx.saved
        out, = ctx.saved_tensors
        g_levels, g_freq, g_phase, g_params, g_pts = query_backward(ctx.net, levels, fr, ph, pts, out, _f32(grad_out), ctx.drop,
                                                                    want_points=ctx.needs_input_grad[5])
        g_vols = g_levels if ctx.vols_channel_last else _caller_format(g_levels, ctx.vol_is_cl)
        return (None, None, None, g_freq, g_phase, g_pts, None, *g_vols, *g_params)


# ---------------------------------------------------------------------------------------------------------------------
# ray batches: the render on caller-given rays (cnerf_render_rays_forward / _backward) as one autograd node
# ---------------------------------------------------------------------------------------------------------------------
RAY_RNG_KEYS = ("u_strat", "eps_coarse", "u_fine", "eps_final", "fine_z")


def _rays_struct(origins, dirs):
    r = L.Rays()
    r.origins, r.dirs = L.ptr(origins).value, L.ptr(dirs).value
    return r


def _rays_cfg(net, o, levels, precision=None, rng=None):
    return make_cfg(net, o["B"], levels, 1, o["S"], 30.0, o["ray_start"], o["ray_end"], o["noise_std"], o["hier"], o["white_back"], o["last_back"],
                    o["clamp_mode"], precision=precision, philox=(rng or {}).get("philox"))


class OccupancyGrid(NamedTuple):
    """One occupancy grid per image: bits (B, G^3 / 32) int32 on the device -- bit (ix G + iy) G + iz of an image in word idx >> 5, bit
    idx & 31 -- over the axis-aligned cube with corner lo (3 floats) and edge side.  include/cnerf.h states what a set bit means."""
    bits: torch.Tensor
    lo: tuple
    side: float
    G: int


def _occ_struct(grid, B):
    bits = grid.bits
    G = int(grid.G)
    if bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[0] != B or bits.shape[1] * 32 != G ** 3:
        raise L.CnerfError(f"occupancy bits must be int32 (B={B}, G^3/32={G ** 3 // 32}), got {bits.dtype} {tuple(bits.shape)}")
    oc = L.Occupancy()
    oc.bits, oc.G, oc.side = L.ptr(bits).value, G, float(grid.side)
    oc.lo = _float3(grid.lo)
    return oc


def occupancy_build(sigma, G, threshold=0.0, dilate=1):
    """cnerf_occupancy_build: sigma (B, (G+1)^3), the density at the cell corners (index (ix (G+1) + iy) (G+1) + iz) -> bits (B, G^3 / 32)
    int32.  A cell's bit is set iff the maximum over the corners of the cells within `dilate` of it is not <= threshold (a NaN sets it)."""
    sigma = _f32(sigma)
    G = int(G)
    if sigma.dim() != 2 or sigma.shape[1] != (G + 1) ** 3:
        raise L.CnerfError(f"occupancy_build: sigma must be (B, (G+1)^3 = {(G + 1) ** 3}), got {tuple(sigma.shape)}")
    B = sigma.shape[0]
    bits = torch.empty((B, max(G, 0) ** 3 // 32), dtype=torch.int32, device=sigma.device)
    L.check(L.lib().cnerf_occupancy_build(B, G, int(dilate), float(threshold), L.ptr(sigma), C.c_void_p(bits.data_ptr()), _stream()),
            "cnerf_occupancy_build")
    return bits


def occupancy_compact(grid, points, rank=None, live_points=None):
    """cnerf_occupancy_compact: points (B,n,3) -> rank (B,n) int32 (index among the image's live points, -1 = skipped), live_points
    (B,n,3) with image b's live positions at the front of its rows, counts (B) int32 on the device.  rank / live_points: buffers to
    write into (the rows of live_points behind counts[b] are left as they are)."""
    points = _f32(points)
    B, n = points.shape[0], points.shape[1]
    dev = points.device
    oc = _occ_struct(grid, B)
    ws = _workspace("cnerf_occupancy_compact_bytes", dev, B, n)
    rank = torch.empty((B, n), dtype=torch.int32, device=dev) if rank is None else rank
    live_points = torch.empty((B, n, 3), dtype=torch.float32, device=dev) if live_points is None else live_points
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    L.check(L.lib().cnerf_occupancy_compact(C.byref(oc), B, n, L.ptr(points), L.ptr(rank), L.ptr(live_points), L.ptr(counts), L.ptr(ws), _stream()),
            "cnerf_occupancy_compact")
    return rank, live_points, counts


def occupancy_expand(rank, live_rgb_sigma, out=None):
    """cnerf_occupancy_expand: rank (B,n) int32, live_rgb_sigma (B,n,4) -> rgb_sigma (B,n,4): the live values at their samples,
    (0, 0, 0, -inf) where the sample was skipped."""
    live_rgb_sigma = _f32(live_rgb_sigma)
    B, n = rank.shape
    out = torch.empty((B, n, 4), dtype=torch.float32, device=rank.device) if out is None else out
    L.check(L.lib().cnerf_occupancy_expand(B, n, L.ptr(rank), L.ptr(live_rgb_sigma), L.ptr(out), _stream()), "cnerf_occupancy_expand")
    return out


def _ray_bounds(near, far, B, P):
    """near / far as render_rays takes them -> detached float32 (B,P) tensors, or (None, None).  ValueError: only one given, a shape other
    than (B,P)."""
    if near is None and far is None:
        return None, None
    if near is None or far is None:
        raise ValueError("render_rays: near and far must both be given, or neither")
    near, far = _f32(near.detach()), _f32(far.detach())
    if tuple(near.shape) != (B, P) or tuple(far.shape) != (B, P):
        raise ValueError(f"render_rays: near and far must both be (B,P) = ({B}, {P}), got {tuple(near.shape)} and {tuple(far.shape)}")
    return near, far


def occupancy_ray_bounds(grid, origins, dirs, t_min, t_max, pad=0.0):
    """cnerf_occupancy_ray_bounds: origins / dirs (B,P,3), one grid per image -> near, far (B,P) float32 and hit (B,P) uint8: the span of
    [t_min, t_max] over which the ray crosses set cells, widened by pad (t and pad in units of |dir|); a ray that crosses none has
    hit = 0 and keeps [t_min, t_max].  Outside the grid's cube a ray counts as empty.  include/cnerf.h states the contract."""
    origins, dirs = _f32(origins.detach()), _f32(dirs.detach())
    if origins.dim() != 3 or origins.shape[-1] != 3 or dirs.shape != origins.shape:
        raise L.CnerfError(f"occupancy_ray_bounds: origins and dirs must both be (B,P,3), got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    B, P = int(origins.shape[0]), int(origins.shape[1])
    oc, rs = _occ_struct(grid, B), _rays_struct(origins, dirs)
    near = torch.empty((B, P), dtype=torch.float32, device=origins.device)
    far = torch.empty_like(near)
    hit = torch.empty((B, P), dtype=torch.uint8, device=origins.device)
    L.check(L.lib().cnerf_occupancy_ray_bounds(C.byref(oc), C.byref(rs), B, P, float(t_min), float(t_max), float(pad), L.ptr(near), L.ptr(far),
                                               C.c_void_p(hit.data_ptr()), _stream()), "cnerf_occupancy_ray_bounds")
    return near, far, hit


def isosurface(values, level, lo=(0.0, 0.0, 0.0), pitch=1.0, attrs=None):
    """cnerf_isosurface_count / _emit: the level set of a scalar lattice values (N0,N1,N2) as an indexed triangle mesh, by marching
    tetrahedra (include/cnerf.h states the algorithm: orderings, arithmetic and orientation are fixed).  Lattice point (i0,i1,i2) sits at
    i * pitch + lo; attrs (N0,N1,N2,C), C <= 8, are interpolated along the edges like the positions.
    -> vertices (Nv,3) float32, faces (Nt,3) int32, vertex_attrs (Nv,C) float32 or None, on the device of `values`.  The two counts are
    copied to the host between the calls (one synchronisation); an empty surface gives empty tensors and no second launch."""
    values = _f32(values.detach())
    if values.dim() != 3:
        raise L.CnerfError(f"isosurface: values must be (N0,N1,N2), got {tuple(values.shape)}")
    n0, n1, n2 = (int(s) for s in values.shape)
    dev = values.device
    if attrs is not None:
        attrs = _f32(attrs.detach())
        if attrs.dim() != 4 or tuple(attrs.shape[:3]) != (n0, n1, n2):
            raise L.CnerfError(f"isosurface: attrs must be ({n0},{n1},{n2},C), got {tuple(attrs.shape)}")
    n_attr = 0 if attrs is None else int(attrs.shape[3])
    lib = L.lib()
    ws = _workspace("cnerf_isosurface_bytes", dev, n0, n1, n2)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    L.check(lib.cnerf_isosurface_count(n0, n1, n2, L.ptr(values), float(level), L.ptr(counts), L.ptr(ws), _stream()), "cnerf_isosurface_count")
    nv, nt = (int(c) for c in counts.tolist())
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    vertex_attrs = None if attrs is None else torch.empty((nv, n_attr), dtype=torch.float32, device=dev)
    if nv == 0:
        return vertices, faces, vertex_attrs
    L.check(lib.cnerf_isosurface_emit(n0, n1, n2, L.ptr(values), float(level), _float3(lo), float(pitch), L.ptr(attrs), n_attr, nv, nt, L.ptr(vertices),
                                      L.ptr(vertex_attrs), L.ptr(faces), L.ptr(ws), _stream()), "cnerf_isosurface_emit")
    return vertices, faces, vertex_attrs


def _lattice(values, who):
    """values as a components call takes them -> detached contiguous float32 (N0,N1,N2) and its three sizes."""
    values = _f32(values.detach())
    if values.dim() != 3:
        raise L.CnerfError(f"{who}: values must be (N0,N1,N2), got {tuple(values.shape)}")
    return values, tuple(int(s) for s in values.shape)


def connected_components(values, level, invert=False, connectivity=14):
    """cnerf_components_label: the connected components of the points of a scalar lattice values (N0,N1,N2) that are INSIDE (v > level,
    the rule of isosurface; invert=True: of all the others).  connectivity=14 joins points that differ by +-(d0,d1,d2), d in {0,1}^3 \\ 0:
    the edges isosurface puts vertices on, so the components are the pieces its mesh separates; 6 is the axis neighbourhood.
    -> labels (N0,N1,N2) int32 (-1 where not selected, else the smallest flat index of the component), sizes (N0,N1,N2) int32 (the point
    count at each root, 0 elsewhere), stats int32[4] (components, root and size of the largest, status) -- all on the device, nothing is
    read back here: stats[3] != 0 says that a loop cap was hit and the rest is not to be used.  include/cnerf.h states the contract."""
    values, (n0, n1, n2) = _lattice(values, "connected_components")
    dev = values.device
    ws = _workspace("cnerf_components_bytes", dev, n0, n1, n2)
    labels = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev)
    sizes = torch.empty_like(labels)
    stats = torch.empty((4,), dtype=torch.int32, device=dev)
    L.check(L.lib().cnerf_components_label(n0, n1, n2, L.ptr(values), float(level), int(bool(invert)), int(connectivity), L.ptr(labels), L.ptr(sizes),
                                           L.ptr(stats), L.ptr(ws), _stream()), "cnerf_components_label")
    return labels, sizes, stats


def keep_components(values, level, largest=True, min_size=0, fill=None, invert=False, connectivity=14, return_labels=False):
    """connected_components, then cnerf_components_filter: the lattice with every selected component that is not the largest (largest=True)
    or has fewer than min_size points overwritten by `fill`, which puts it on the other side of the level: None stands for -inf (+inf with
    invert); a fill on the selected side (> level without invert, not > level with it) is a ValueError.  All else is copied; with
    connectivity 14, isosurface of the result is the mesh of `values` less the sheets of those components, bit for bit.
    -> the filtered (N0,N1,N2) float32 lattice, a new tensor; with return_labels also labels, sizes, stats of connected_components.
    Nothing is read back from the device."""
    values, (n0, n1, n2) = _lattice(values, "keep_components")
    if fill is None:
        fill = float("inf") if invert else float("-inf")
    fill = C.c_float(fill).value                                  # as the C call rounds it, and the level beside it
    if fill != fill or (fill > C.c_float(level).value) != bool(invert):
        raise ValueError(f"keep_components: fill={fill} must{'' if invert else ' not'} be > level={level} with invert={bool(invert)}")
    labels, sizes, stats = connected_components(values, level, invert=invert, connectivity=connectivity)
    out = torch.empty_like(values)
    L.check(L.lib().cnerf_components_filter(n0, n1, n2, L.ptr(values), L.ptr(labels), L.ptr(sizes), L.ptr(stats), int(bool(largest)), int(min_size), fill,
                                            L.ptr(out), _stream()), "cnerf_components_filter")
    return (out, labels, sizes, stats) if return_labels else out


def _cloud_lengths(lengths, B, dev, what, who="nearest_points"):
    """Per-image lengths of a padded cloud -> contiguous int32 (B,) on `dev`, or None."""
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths).detach().to(device=dev, dtype=torch.int32).contiguous()
    if tuple(lengths.shape) != (B,):
        raise L.CnerfError(f"{who}: {what} must be ({B},), got {tuple(lengths.shape)}")
    return lengths


def nearest_points(queries, targets, query_lengths=None, target_lengths=None, target_splits=0):
    """cnerf_nearest_points: for every query the nearest target of the same image, exactly (brute force; include/cnerf.h states the
    arithmetic, the lowest-index tie rule and the treatment of non-finite values).  queries (B,n,3), targets (B,m,3); query_lengths /
    target_lengths (B,) say how many leading rows of each image count (clamped to [0,n] / [0,m]; None: all).
    -> dist2 (B,n) float32 squared distances, idx (B,n) int32; (+inf, -1) where no target can be chosen and in rows beyond the length.
    (n,3) and (m,3) are taken as one image and returned without the batch axis.  target_splits: 0 lets the library choose; the result
    does not depend on it.  Inputs are detached: shape_metrics.chamfer_distance is the differentiable form."""
    queries, targets = _f32(queries.detach()), _f32(targets.detach())
    single = queries.dim() == 2 and targets.dim() == 2
    if single:
        queries, targets = queries.unsqueeze(0), targets.unsqueeze(0)
    if queries.dim() != 3 or targets.dim() != 3 or queries.shape[-1] != 3 or targets.shape[-1] != 3 or queries.shape[0] != targets.shape[0]:
        raise L.CnerfError(f"nearest_points: queries and targets must be (B,n,3) and (B,m,3) (or (n,3) and (m,3)), got {tuple(queries.shape)} "
                           f"and {tuple(targets.shape)}")
    if targets.device != queries.device:
        raise L.CnerfError("nearest_points: queries and targets must be on the same device")
    B, n, m = int(queries.shape[0]), int(queries.shape[1]), int(targets.shape[1])
    dev = queries.device
    nq = _cloud_lengths(query_lengths, B, dev, "query_lengths")
    mt = _cloud_lengths(target_lengths, B, dev, "target_lengths")
    ws = _workspace("cnerf_nearest_points_bytes", dev, B, n, m, int(target_splits))
    dist2 = torch.empty((B, n), dtype=torch.float32, device=dev)
    idx = torch.empty((B, n), dtype=torch.int32, device=dev)
    L.check(L.lib().cnerf_nearest_points(B, n, m, L.ptr(queries), L.ptr(targets), L.ptr(nq), L.ptr(mt), int(target_splits), L.ptr(dist2), L.ptr(idx),
                                         L.ptr(ws), _stream()), "cnerf_nearest_points")
    return (dist2[0], idx[0]) if single else (dist2, idx)


VOXEL_LAYOUTS = {"encoder": 0, "npz": 1}


def _voxel_layout(layout, who):
    if layout not in VOXEL_LAYOUTS:
        raise L.CnerfError(f"{who}: layout must be 'encoder' (B,4,G,G,G) or 'npz' (B,G,G,G,4), got {layout!r}")
    return VOXEL_LAYOUTS[layout]


def voxelize(points, G, lo, side, lengths=None, clip_margin=1e-4, layout="encoder", want_counts=False):
    """cnerf_voxelize: a coloured cloud points (B,n,stride >= 6) = [x, y, z, r, g, b, ...] -> the voxel grid [occupancy, r, g, b] over the
    cube with corner lo (a number or three) and edge side, G cells per axis: occupancy 1 where a point fell, the mean of the points'
    colours (clamped to [0,1]) beside it, 0 in empty cells.  layout "encoder": (B,4,G,G,G) indexed [b, ch, iz, iy, ix], what the U-Net
    takes; "npz": (B,G,G,G,4) indexed [b, ix, iy, iz, ch], the order of voxel.npz.  lengths (B,): how many leading rows of each image
    count (clamped to [0,n]; None: all).  clip_margin >= 0 clamps coordinates into [lo + m, lo + side - m] first (the reference's 1e-4);
    None or < 0: points outside the cube are skipped.  A point with a NaN coordinate is always skipped.
    -> voxels float32, and counts int32 (B,G,G,G) in the layout's spatial order with want_counts.  (n,stride) is taken as one image and
    returned without the batch axis.  The colour sums are exact integers (include/cnerf.h): two calls give the same bits.
    Forward only: the input is detached, the outputs carry no gradient."""
    if not points.is_cuda:
        raise L.CnerfError("voxelize: points must be on the GPU (there is no CPU fallback)")
    points = _f32(points.detach())
    single = points.dim() == 2
    if single:
        points = points.unsqueeze(0)
    if points.dim() != 3 or points.shape[-1] < 6:
        raise L.CnerfError(f"voxelize: points must be (B,n,6 or more) (or (n,6 or more)), got {tuple(points.shape)}")
    code = _voxel_layout(layout, "voxelize")
    B, n, stride = (int(s) for s in points.shape)
    G = int(G)
    dev = points.device
    np_ = _cloud_lengths(lengths, B, dev, "lengths", "voxelize")
    ws = _workspace("cnerf_voxelize_bytes", dev, B, G)
    voxels = torch.empty((B, 4, G, G, G) if code == 0 else (B, G, G, G, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((B, G, G, G), dtype=torch.int32, device=dev) if want_counts else None
    margin = -1.0 if clip_margin is None else float(clip_margin)
    L.check(L.lib().cnerf_voxelize(B, n, stride, L.ptr(points), L.ptr(np_), G, _float3(lo), float(side), margin, code, L.ptr(voxels), L.ptr(counts),
                                   L.ptr(ws), _stream()), "cnerf_voxelize")
    if single:
        voxels, counts = voxels[0], (counts[0] if want_counts else None)
    return (voxels, counts) if want_counts else voxels


def voxel_first_hit(voxels, origins, dirs, lo, side, t_min, t_max, num_steps, background=(1.0, 1.0, 1.0), layout="encoder"):
    """cnerf_voxel_first_hit: the picture of a voxel grid.  Along every ray o + t d, at the num_steps depths of
    torch.linspace(t_min, t_max, num_steps), the colour of the first sample that lies in a cell with occupancy != 0; the background
    where there is none.  A sample outside the cube sees nothing.  voxels (B,4,G,G,G) ("encoder") or (B,G,G,G,4) ("npz"); origins, dirs
    (B,P,3), directions not normalised.
    -> pixels (B,P,3) in the grid's own colour range, hit_t (B,P) float32 (+inf: no hit), hit_cell (B,P) int32 = (ix G + iy) G + iz
    (-1: no hit).  A single grid with (P,3) rays is taken as one image and returned without the batch axis.
    Forward only: the inputs are detached, the outputs carry no gradient."""
    if not (voxels.is_cuda and origins.is_cuda and dirs.is_cuda):
        raise L.CnerfError("voxel_first_hit: voxels, origins and dirs must be on the GPU (there is no CPU fallback)")
    voxels, origins, dirs = _f32(voxels.detach()), _f32(origins.detach()), _f32(dirs.detach())
    code = _voxel_layout(layout, "voxel_first_hit")
    single = voxels.dim() == 4 and origins.dim() == 2
    if single:
        voxels, origins, dirs = voxels.unsqueeze(0), origins.unsqueeze(0), dirs.unsqueeze(0)
    ok = voxels.dim() == 5 and voxels.shape[1 if code == 0 else 4] == 4 and len({int(voxels.shape[k]) for k in ((2, 3, 4) if code == 0 else (1, 2, 3))}) == 1
    if not ok:
        raise L.CnerfError(f"voxel_first_hit: voxels must be (B,4,G,G,G) ('encoder') or (B,G,G,G,4) ('npz'), got {tuple(voxels.shape)} as {layout!r}")
    if origins.dim() != 3 or origins.shape[-1] != 3 or dirs.shape != origins.shape or origins.shape[0] != voxels.shape[0]:
        raise L.CnerfError(f"voxel_first_hit: origins and dirs must both be (B={voxels.shape[0]},P,3), got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    if origins.device != voxels.device or dirs.device != voxels.device:
        raise L.CnerfError("voxel_first_hit: voxels, origins and dirs must be on the same device")
    B, P, G = int(origins.shape[0]), int(origins.shape[1]), int(voxels.shape[2])
    dev = voxels.device
    pixels = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    hit_t = torch.empty((B, P), dtype=torch.float32, device=dev)
    hit_cell = torch.empty((B, P), dtype=torch.int32, device=dev)
    rs = _rays_struct(origins, dirs)
    L.check(L.lib().cnerf_voxel_first_hit(B, P, C.byref(rs), L.ptr(voxels), G, _float3(lo), float(side), code, float(t_min), float(t_max),
                                          int(num_steps), _float3(background), L.ptr(pixels), L.ptr(hit_t), L.ptr(hit_cell), _stream()), "cnerf_voxel_first_hit")
    return (pixels[0], hit_t[0], hit_cell[0]) if single else (pixels, hit_t, hit_cell)


COLOR_LAYOUTS = {"chw": 0, "hwc": 1}


def _cams16(cam2worlds, lead, who):
    """cam2world matrices (*lead,4,4) or (*lead,16) -> contiguous float32 (*lead,16)."""
    c = _f32(cam2worlds.detach())
    if tuple(c.shape) == tuple(lead) + (4, 4):
        c = c.reshape(*lead, 16)
    if tuple(c.shape) != tuple(lead) + (16,):
        raise L.CnerfError(f"{who}: cam2worlds must be {tuple(lead) + (4, 4)}, got {tuple(cam2worlds.shape)}")
    return c.contiguous()


def _view_inputs(who, depth, cam2worlds, colors, color_layout, mask=None):
    """What backproject and tsdf_integrate take alike: depth maps (V,R,R), their cameras, colours in `color_layout` or None, a mask or None
    -> (depth, cams, colors, mask) detached, float32 and on one device, and (V, R, the layout's code, the device)."""
    if not (depth.is_cuda and cam2worlds.is_cuda):
        raise L.CnerfError(f"{who}: depth and cam2worlds must be on the GPU (there is no CPU fallback)")
    depth = _f32(depth.detach())
    if depth.dim() != 3 or depth.shape[1] != depth.shape[2]:
        raise L.CnerfError(f"{who}: depth must be (V,R,R), got {tuple(depth.shape)}")
    if color_layout not in COLOR_LAYOUTS:
        raise L.CnerfError(f"{who}: color_layout must be 'chw' (V,3,R,R) or 'hwc' (V,R,R,3), got {color_layout!r}")
    code = COLOR_LAYOUTS[color_layout]
    V, R = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    cams = _cams16(cam2worlds, (V,), who)
    if colors is not None:
        colors = _f32(colors.detach())
        if tuple(colors.shape) != ((V, 3, R, R) if code == 0 else (V, R, R, 3)):
            raise L.CnerfError(f"{who}: colors must be {(V, 3, R, R) if code == 0 else (V, R, R, 3)} as {color_layout!r}, got {tuple(colors.shape)}")
    if mask is not None:
        mask = _f32(mask.detach())
        if mask.shape != depth.shape:
            raise L.CnerfError(f"{who}: mask must be {tuple(depth.shape)}, got {tuple(mask.shape)}")
    if any(t is not None and t.device != dev for t in (cams, colors, mask)):
        raise L.CnerfError(f"{who}: all tensors must be on the same device")
    return (depth, cams, colors, mask), (V, R, code, dev)


def backproject(depth, cam2worlds, focal, z_min, z_max, colors=None, color_layout="chw", color_scale=1.0, color_offset=0.0, mask=None, mask_min=0.0,
                want_pixel=False, want_rank=False):
    """cnerf_backproject: V depth maps (V,R,R) with their cameras (V,4,4) -> ONE cloud in world space.  A pixel is valid iff
    z_min < depth < z_max (both strict, a NaN is not) and, with mask (V,R,R), mask > mask_min; a valid pixel gives the row
    [x, y, z] -- [x, y, z, r, g, b] with colors, (V,3,R,R) as "chw" (the generator's pixels) or (V,R,R,3) as "hwc", each channel
    c * color_scale + color_offset -- and the rows come in ascending (view, row, col).  focal: 1 / tan(fov / 2) in fp32, as
    volumetric_rendering.pinhole_rays forms it.
    -> points (n, 6 or 3) float32, counts (V,) int32 on the device (valid pixels per view, summing to n), then with want_pixel
    pixel (n,) int32 = (v R + row) R + col of every row, and with want_rank rank (V,R,R) int32 = the pixel's row in the cloud or -1.
    Reading n back is the one synchronisation.  Forward only: the inputs are detached, the outputs carry no gradient."""
    (depth, cams, colors, mask), (V, R, code, dev) = _view_inputs("backproject", depth, cam2worlds, colors, color_layout, mask)
    ws = _workspace("cnerf_backproject_bytes", dev, V, R)
    points = torch.empty((V * R * R, 6 if colors is not None else 3), dtype=torch.float32, device=dev)
    counts = torch.empty((V,), dtype=torch.int32, device=dev)
    pixel = torch.empty((V * R * R,), dtype=torch.int32, device=dev) if want_pixel else None
    rank = torch.empty((V, R, R), dtype=torch.int32, device=dev) if want_rank else None
    L.check(L.lib().cnerf_backproject(V, R, L.ptr(depth), L.ptr(colors), code, L.ptr(mask), float(mask_min), L.ptr(cams), float(focal), float(z_min),
                                      float(z_max), float(color_scale), float(color_offset), L.ptr(points), L.ptr(counts), L.ptr(pixel), L.ptr(rank),
                                      L.ptr(ws), _stream()), "cnerf_backproject")
    n = int(counts.sum().item())
    out = (points[:n], counts)
    if want_pixel:
        out += (pixel[:n],)
    if want_rank:
        out += (rank,)
    return out


def splat_points(points, cam2worlds, R, focal, z_min, z_max, radius=0, lengths=None, background=(1.0, 1.0, 1.0), want_pixels=True):
    """cnerf_splat_points: the z-buffered picture of a cloud.  points (B,n,stride >= 3) = [x, y, z, (r, g, b, ...)] in world space,
    cam2worlds (B,V,4,4) with rotations in their 3x3 blocks.  A point with camera-space depth z_min < z < z_max lands on the pixel
    nearest to its projection and covers the (2 radius + 1)^2 pixels around it; per pixel the nearest point wins, at equal depth the
    lowest index.  lengths (B,): how many leading rows of each cloud count.
    -> depth (B,V,R,R) float32, 0 where nothing landed; index (B,V,R,R) int32, the winner's row or -1; pixels (B,V,R,R,3), the
    winner's colour as stored or `background` (None with want_pixels=False; colours need stride >= 6).  The result is the same
    bits on every run.  Forward only: the inputs are detached, the outputs carry no gradient."""
    if not (points.is_cuda and cam2worlds.is_cuda):
        raise L.CnerfError("splat_points: points and cam2worlds must be on the GPU (there is no CPU fallback)")
    points = _f32(points.detach())
    if points.dim() != 3 or points.shape[-1] < 3:
        raise L.CnerfError(f"splat_points: points must be (B,n,3 or more), got {tuple(points.shape)}")
    B, n, stride = (int(s) for s in points.shape)
    if cam2worlds.dim() < 3 or cam2worlds.shape[0] != B:
        raise L.CnerfError(f"splat_points: cam2worlds must be (B={B},V,4,4), got {tuple(cam2worlds.shape)}")
    V, R = int(cam2worlds.shape[1]), int(R)
    cams = _cams16(cam2worlds, (B, V), "splat_points")
    dev = points.device
    if cams.device != dev:
        raise L.CnerfError("splat_points: points and cam2worlds must be on the same device")
    np_ = _cloud_lengths(lengths, B, dev, "lengths", "splat_points")
    ws = _workspace("cnerf_splat_points_bytes", dev, B, V, R)
    depth = torch.empty((B, V, R, R), dtype=torch.float32, device=dev)
    index = torch.empty((B, V, R, R), dtype=torch.int32, device=dev)
    pixels = torch.empty((B, V, R, R, 3), dtype=torch.float32, device=dev) if want_pixels else None
    L.check(L.lib().cnerf_splat_points(B, n, stride, L.ptr(points), L.ptr(np_), V, L.ptr(cams), R, float(focal), float(z_min), float(z_max), int(radius),
                                       _float3(background), L.ptr(depth), L.ptr(index), L.ptr(pixels), L.ptr(ws), _stream()), "cnerf_splat_points")
    return depth, index, pixels


def tsdf_integrate(depth, cam2worlds, focal, z_min, z_max, shape, lo, pitch, trunc, colors=None, color_layout="chw", color_scale=1.0, color_offset=0.0,
                   carve=True, hidden_min=1, unseen=-1.0, want_weight=False):
    """cnerf_tsdf_integrate: V depth maps (V,R,R) with their cameras (V,4,4) -> a truncated signed distance lattice of `shape`
    (n0,n1,n2), point (i0,i1,i2) at i * pitch + lo with lattice axis c = world axis c -- the lattice rule of ops.isosurface, not
    extract_mesh's reversed columns.  Every voxel is projected into every view and reads the nearest pixel's depth d: with
    z_min < d < z_max the view observes s = (z - d) / trunc clamped below at -1 (positive BEHIND the surface), or counts the voxel as
    hidden when s > 1; any other depth but a NaN is background and, with carve, observes -1.  tsdf is the mean of the observations;
    without one it is 1 where at least hidden_min > 0 views hid the voxel, else `unseen`.  include/cnerf.h states the arithmetic.
    colors: (V,3,R,R) as "chw" (the generator's pixels) or (V,R,R,3) as "hwc", each channel c * color_scale + color_offset.
    -> tsdf (n0,n1,n2) float32; weight (n0,n1,n2) int32 with want_weight, else None: the observations, or minus the hiding views, 0 where
    no view says anything; rgb (n0,n1,n2,3) float32 with colors, else None: the mean colour of the observations within the band, 0
    where there is none.  ops.isosurface(tsdf, 0.0, lo, pitch, attrs=rgb) meshes it, normals outward.  The same bits on every run; no
    synchronisation.  Forward only: the inputs are detached, the outputs carry no gradient."""
    (depth, cams, colors, _), (V, R, code, dev) = _view_inputs("tsdf_integrate", depth, cam2worlds, colors, color_layout)
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3:
        raise L.CnerfError(f"tsdf_integrate: shape must be (n0,n1,n2), got {shape}")
    # refusals come before any allocation: a lattice of a refused shape is never sized
    if any(s < 2 or s > 1024 for s in shape) or shape[0] * shape[1] * shape[2] > 1 << 27:
        raise L.CnerfError(f"tsdf_integrate: shape {shape} must have every n in [2,1024] and at most 2^27 points")
    tsdf = torch.empty(shape, dtype=torch.float32, device=dev)
    weight = torch.empty(shape, dtype=torch.int32, device=dev) if want_weight else None
    rgb = torch.empty(shape + (3,), dtype=torch.float32, device=dev) if colors is not None else None
    L.check(L.lib().cnerf_tsdf_integrate(*shape, _float3(lo), float(pitch), V, R, L.ptr(depth), L.ptr(colors), code, float(color_scale),
                                         float(color_offset), L.ptr(cams), float(focal), float(z_min), float(z_max), float(trunc), int(bool(carve)),
                                         int(hidden_min), float(unseen), L.ptr(tsdf), L.ptr(weight), L.ptr(rgb), _stream()), "cnerf_tsdf_integrate")
    return tsdf, weight, rgb


def render_rays_forward(net, levels, freq, phase, origins, dirs, o, rng=None, want_aux=False, aux_keys=None, occupancy=None, near=None, far=None):
    """cnerf_render_rays_forward on channel-last levels: origins / dirs (B,P,3) -> pixels (B,P,3), dist (B,P), aux dict.
    occupancy (an OccupancyGrid with one grid per image): cnerf_render_rays_masked_forward instead -- samples in cells whose bit is
    clear are not evaluated; forward only; the call synchronises the stream.  aux then also holds live_coarse / live_fine, (B,) int32
    on the host: the points each pass gave to the field.
    near / far (B,P): the coarse samples of ray (b,p) are placed over [near, far] instead of [ray_start, ray_end] (the bounded entries);
    without them the call is what it was."""
    origins, dirs = _f32(origins), _f32(dirs)
    if origins.dim() != 3 or origins.shape[-1] != 3 or dirs.shape != origins.shape:
        raise L.CnerfError(f"render_rays: origins and dirs must both be (B,P,3), got {tuple(origins.shape)} and {tuple(dirs.shape)}")
    near, far = _ray_bounds(near, far, o["B"], int(origins.shape[1]))
    bounds = None
    if near is not None:
        bounds = L.RayBounds()
        bounds.near, bounds.far = L.ptr(near).value, L.ptr(far).value
    B, P, S, hier = o["B"], int(origins.shape[1]), o["S"], o["hier"]
    n = 2 * S if hier else S
    dev = origins.device
    cfg = _rays_cfg(net, o, levels, rng=rng)
    packed = pack_field(net, cfg)
    ws = _workspace("cnerf_render_rays_workspace_bytes" if occupancy is None else "cnerf_render_rays_masked_workspace_bytes", dev, C.byref(cfg), P)
    pixels = torch.empty((B, P, 3), dtype=torch.float32, device=dev)
    dist = torch.empty((B, P), dtype=torch.float32, device=dev)
    r, keep = _rng_struct(rng or {}, RAY_RNG_KEYS)
    aux_t, aux_s = _aux_buffers(want_aux, aux_keys, B, P, S, n, hier, dev)
    vs, rs = volumes_struct(levels), _rays_struct(origins, dirs)
    # one entry per combination of bounds and occupancy; their arguments differ in those pieces only
    entry = "cnerf_render_rays_" + ("bounded_" if bounds is not None else "") + ("masked_" if occupancy is not None else "") + "forward"
    args = [C.byref(cfg), C.byref(rs), P]
    if bounds is not None:
        args.append(C.byref(bounds))
    if occupancy is not None:
        oc = _occ_struct(occupancy, B)
        live = (C.c_int32 * (2 * B))()
        args.append(C.byref(oc))
    args += [C.byref(vs), L.ptr(packed), L.ptr(_f32(freq)), L.ptr(_f32(phase)), C.byref(r), L.ptr(pixels), L.ptr(dist),
             C.byref(aux_s) if aux_s is not None else None]
    if occupancy is not None:
        args.append(live)
    L.check(getattr(L.lib(), entry)(*args, L.ptr(ws), _stream()), entry)
    if occupancy is not None and (want_aux or aux_keys):
        aux_t["live_coarse"] = torch.tensor(live[:B], dtype=torch.int32)
        if hier:
            aux_t["live_fine"] = torch.tensor(live[B:], dtype=torch.int32)
    return pixels, dist, aux_t


def render_rays_backward(net, o, levels, freq, phase, origins, dirs, rng, saved, grad_pixels, grad_dist, want_rays):
    """Gradients of one ray render w.r.t. (channel-last volume levels, freq, phase, field parameters, origins, dirs): ONE call into the
    library (cnerf_render_rays_backward); its field passes are chunked like a field query's (query_chunk)."""
    global LAST_SATURATED
    B, P, S, hier = o["B"], int(origins.shape[1]), o["S"], o["hier"]
    dev = origins.device
    bprec = backward_precision_of(net)
    pfilm32 = net.spec.layers[0] == "pfilm" and bprec == "fp32"
    cfg = _rays_cfg(net, o, levels, precision="fp16x3" if bprec == "fp16" else ("fp32" if pfilm32 else None), rng=rng)
    w = _backward_setup(net, cfg, levels, B, dev)
    g_org = torch.zeros_like(origins) if want_rays[0] else None
    g_dir = torch.zeros_like(dirs) if want_rays[1] else None

    def bytes_of(ppc):
        nb = C.c_size_t(0)
        L.check(L.lib().cnerf_render_rays_backward_workspace_bytes(C.byref(cfg), w.code, P, int(ppc), C.byref(nb)), "cnerf_render_rays_backward_workspace_bytes")
        return nb.value

    ppc, ws_bytes = query_chunk(P * S, bytes_of, dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    r, keep = _rng_struct(rng, ("u_strat", "eps_final"))
    c_rs, c_z, f_rs, f_z = saved[:4]
    sv = L.Saved()
    sv.coarse_rgb_sigma, sv.coarse_z = L.ptr(c_rs).value, L.ptr(c_z).value
    if hier:
        sv.fine_rgb_sigma, sv.fine_z = L.ptr(f_rs).value, L.ptr(f_z).value
    rs = _rays_struct(origins, dirs)
    L.check(L.lib().cnerf_render_rays_backward(C.byref(cfg), w.code, ppc, C.byref(rs), P, C.byref(w.vs), C.byref(w.fp), L.ptr(w.packed), L.ptr(w.packed_bwd),
                                               L.ptr(freq), L.ptr(phase), C.byref(r), C.byref(sv), L.ptr(_f32(grad_pixels)), L.ptr(_f32(grad_dist)),
                                               C.byref(w.gp), L.ptr(w.g_freq), L.ptr(w.g_phase), C.byref(w.gvs), L.ptr(g_org), L.ptr(g_dir), L.ptr(w.sat),
                                               L.ptr(ws), _stream()), "cnerf_render_rays_backward")
    if w.sat is not None:
        LAST_SATURATED = w.sat
    return w.grad_levels, w.g_freq, w.g_phase, w.grads, g_org, g_dir


class RenderRaysFunction(torch.autograd.Function):
    """ImplicitGenerator3d.render_rays as one autograd node: differentiable w.r.t. the feature volume(s), freq / phase (and through them
    the mapping network and the global feature), the field parameters and the rays' origins and directions; the sample depths carry no
    gradient (the reference draws and resamples them under no_grad: generators.py:57,111).  Per-ray bounds travel in o["near"] / o["far"],
    detached: they place depths, so they get no gradient either (None in backward, with the rest of `o`); the backward reads the saved
    depths and never the interval."""

    @staticmethod
    def forward(ctx, net, o, rng, origins, dirs, freq, phase, n_vols, *rest):
        vols, params = rest[:n_vols], rest[n_vols:]
        levels = [channel_last(v.detach()) for v in vols]
        ctx.vol_is_cl = _is_channel_last(levels, vols)
        fr = _f32(freq.detach()) if freq is not None else None
        ph = _f32(phase.detach()) if phase is not None else None
        org, drs = _f32(origins.detach()), _f32(dirs.detach())
        need_grad = o["need_grad"]
        pixels, dist, aux = render_rays_forward(net, levels, fr, ph, org, drs, o, rng, want_aux=o["want_aux"],
                                                aux_keys=SAVED_KEYS if need_grad and not o["want_aux"] else None, near=o.get("near"), far=o.get("far"))
        ctx.net, ctx.o, ctx.rng, ctx.n_vols = net, o, rng, n_vols
        if need_grad:
            saved = [aux.get(k) for k in SAVED_KEYS]
            if o["hier"] and rng.get("fine_z") is not None:
                saved[3] = _f32(rng["fine_z"]).reshape(saved[1].shape)   # teacher-forced depths are what the fine pass used
            ctx.saved = (levels, fr, ph, org, drs, tuple(saved))
        RenderRaysFunction.last_aux = aux
        return pixels, dist

    @staticmethod
    def backward(ctx, grad_pixels, grad_dist):
        levels, fr, ph, org, drs, saved = ctx.saved
        g_levels, g_freq, g_phase, g_params, g_org, g_dir = render_rays_backward(
            ctx.net, ctx.o, levels, fr, ph, org, drs, ctx.rng, saved, grad_pixels.contiguous(),
            grad_dist.contiguous() if grad_dist is not None else None, want_rays=ctx.needs_input_grad[3:5])
        g_vols = _caller_format(g_levels, ctx.vol_is_cl)
        return (None, None, None, g_org, g_dir, g_freq, g_phase, None, *g_vols, *g_params)


def render_rays(net, fvol, freq, phase, origins, dirs, ray_start, ray_end, num_steps, hierarchical, clamp_mode, noise_std,
                white_back=False, last_back=False, rng=None, want_aux=False, occupancy=None, near=None, far=None):
    """Differentiable render of caller-given rays, used by ImplicitGenerator3d.render_rays.  origins / dirs (B,P,3) world (dirs are not
    normalised here: depths are in units of |dir|); fvol: (B,C,V,V,V) or a list of pyramid levels.
    occupancy (OccupancyGrid): the masked render -- forward only, no autograd node; refuses inputs that require grad in grad mode.
    near / far (B,P), both or neither: the coarse samples of a ray are placed over its own [near, far] instead of [ray_start, ray_end]
    (occupancy_ray_bounds makes them from a grid), with and without `occupancy`, forward and backward.  They are detached: no gradient
    flows to them, whether or not they require one.  ValueError: only one given, a shape other than (B,P).
    Returns (pixels (B,P,3) = 2*rgb-1, dist (B,P) = distance along the ray, aux dict)."""
    o = dict(B=int(origins.shape[0]), S=int(num_steps), ray_start=float(ray_start), ray_end=float(ray_end), hier=bool(hierarchical),
             clamp_mode=clamp_mode, noise_std=float(noise_std), white_back=bool(white_back), last_back=bool(last_back), want_aux=bool(want_aux))
    _ray_flags(clamp_mode, white_back, last_back)      # refuses an unknown clamp mode before any work
    near, far = _ray_bounds(near, far, o["B"], int(origins.shape[1]))
    vols = as_levels(fvol)
    params = net.field_params()
    o["need_grad"] = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (origins, dirs, freq, phase, *vols, *params))
    if occupancy is not None:
        if o["need_grad"]:
            raise L.CnerfError("render_rays with an occupancy grid is forward only: call it under torch.no_grad()")
        det = lambda t: None if t is None else _f32(t.detach())
        with torch.no_grad():
            return render_rays_forward(net, [channel_last(v.detach()) for v in vols], det(freq), det(phase), det(origins), det(dirs), o, rng or {},
                                       want_aux=want_aux, occupancy=occupancy, near=near, far=far)
    if near is not None:
        o["near"], o["far"] = near, far
    pixels, dist = RenderRaysFunction.apply(net, o, rng or {}, origins, dirs, freq, phase, len(vols), *vols, *params)
    return pixels, dist, (RenderRaysFunction.last_aux if want_aux else {})
