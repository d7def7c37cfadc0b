"""Shared by tests/test_render_rays_cpu.py and tests/test_gpu_render_rays.py: a ray oracle -- the render of caller-given rays
(ImplicitGenerator3d.render_rays, cnerf_render_rays_forward) composed from the stages of oracle/render_oracle.py -- and random cases
for it.  TEST INFRASTRUCTURE ONLY.

The oracle, in the dtype `dt` of the field (float32 or float64):
  1. depths  z = zl[s] + (u - 0.5) (zl[1] - zl[0]),  zl = torch.linspace(ray_start, ray_end, S)      float32, no_grad
  2. positions  o + d * z  (a product, then a sum: two roundings)                                     float32, no_grad
  3. field_eval at them                                                                               dt
  4. composite (coarse weights)                                                                       float32, no_grad
  5. importance_depths                                                                                float32, no_grad
  6. merge_by_depth                                                                                   dt
  7. composite -> pixels = 2 rgb - 1 (B,P,3), dist = sum w z (B,P)                                     dt
The sample depths and the VALUES of the positions carry no gradient and are float32 in both dtypes (the float64 run is "the same
samples, exact arithmetic": the floor of the fp32 one).  When origins / dirs require grad, the positions get their derivative --
d p / d o = 1, d p / d d = z, z a constant (generators.py:57,111 of the reference draw and resample the depths under no_grad) -- by
adding (o - o.detach()) + (d - d.detach()) * z, which is zero in value."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import render_oracle as O

RAY_START, RAY_END = 0.25, 1.95


def ray_depths(u_strat, S, ray_start, ray_end):
    """Step 1: u_strat (B,P,S) -> z (B,P,S), float32."""
    z_lin = torch.linspace(ray_start, ray_end, S)
    return z_lin.reshape(1, 1, S) + (u_strat.float() - 0.5) * (z_lin[1] - z_lin[0])


def ray_points(origins, dirs, z):
    """Step 2: origins, dirs (B,P,3), z (B,P,S) -> (B,P,S,3), float32: the product is rounded, then the sum."""
    return origins.float().unsqueeze(2) + dirs.float().unsqueeze(2) * z.float().unsqueeze(-1)


def _with_ray_gradient(pts32, origins, dirs, z, dt):
    p = pts32.to(dt)
    if origins.requires_grad or dirs.requires_grad:
        p = p + (origins - origins.detach()).unsqueeze(2) + (dirs - dirs.detach()).unsqueeze(2) * z.to(dt).unsqueeze(-1)
    return p


def ray_oracle(field, origins, dirs, S, ray_start, ray_end, hierarchical, clamp, noise, white_back, last_back, u_strat, u_fine=None,
               eps_coarse=None, eps_final=None, forced_fine_z=None, dt=torch.float32):
    """field(points (B,N,3) of dtype dt) -> rgb_sigma (B,N,4).  origins / dirs: dtype dt (leaves that require grad get one).
    Returns (pixels (B,P,3), dist (B,P), aux)."""
    B, P = origins.shape[:2]
    with torch.no_grad():
        z = ray_depths(u_strat.reshape(B, P, S), S, ray_start, ray_end)
        pts = ray_points(origins, dirs, z)
    c_out = field(_with_ray_gradient(pts, origins, dirs, z, dt).reshape(B, P * S, 3)).reshape(B, P, S, 4)
    aux = dict(coarse_z=z, coarse_points=pts, coarse_rgb_sigma=c_out)
    ec = None if eps_coarse is None else eps_coarse.reshape(B, P, S).float()
    ef = None if eps_final is None else eps_final.reshape(B, P, -1).to(dt)
    if hierarchical:
        with torch.no_grad():
            _, _, w = O.composite(c_out.detach().float(), z, ec, noise, clamp)
            fine_z, inds, cdf = O.importance_depths(z, w, u_fine.reshape(B, P, S).float())
            aux.update(coarse_weights=w, cdf=cdf, inds=inds, resampled_z=fine_z)
            if forced_fine_z is not None:
                fine_z = forced_fine_z.reshape(B, P, S).float()
            fpts = ray_points(origins, dirs, fine_z)
        f_out = field(_with_ray_gradient(fpts, origins, dirs, fine_z, dt).reshape(B, P * S, 3)).reshape(B, P, S, 4)
        all_out, all_z, sort_idx = O.merge_by_depth(f_out, c_out, fine_z.to(dt), z.to(dt))
        aux.update(fine_z=fine_z, fine_points=fpts, fine_rgb_sigma=f_out, sort_idx=sort_idx)
    else:
        all_out, all_z = c_out, z.to(dt)
    rgb, dist, wfin = O.composite(all_out, all_z, ef, noise, clamp, white_back, last_back)
    aux.update(final_weights=wfin)
    return rgb * 2 - 1, dist, aux


# ---------------------------------------------------------------------------------------------------------------------
# the field of a generator as the oracle evaluates it
# ---------------------------------------------------------------------------------------------------------------------
def oracle_field(variant, params, vols, glob, dt):
    """points -> rgb_sigma through oracle.render_oracle.field_eval (SHORTSIREN: the restatement of tests/global_latent_common.py: the
    oracle's table has no network without a volume); params / vols / glob already of dtype dt."""
    if variant == "SHORTSIREN":
        from global_latent_common import field as latent_field
        return lambda pts: latent_field(params, glob, pts)

    def run(pts):
        keep = torch.get_default_dtype()
        torch.set_default_dtype(dt)
        try:
            return O.field_eval(O.FIELD_SPECS[variant], params, vols if len(vols) > 1 else vols[0], glob, pts)[0]
        finally:
            torch.set_default_dtype(keep)
    return run


def level_shapes(variant, V):
    """(channels, edge) per volume level."""
    if variant == "SHORTSIREN":
        return []
    return [(32, V), (64, max(V // 2, 2)), (32, max(V // 4, 2))] if variant.endswith("Pyrmd") else [(32, V)]


def random_rays(B, P, seed, unnormalised=False):
    """Origins on spheres of radius 1 - 1.5, aimed at a point within 0.2 of the centre; unit directions, or of length 0.7 - 1.3."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(B, P, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * (1.0 + 0.5 * torch.rand(B, P, 1, generator=g))
    d = (torch.rand(B, P, 3, generator=g) * 2 - 1) * 0.2 - o
    d = d / d.norm(dim=-1, keepdim=True)
    if unnormalised:
        d = d * (0.7 + 0.6 * torch.rand(B, P, 1, generator=g))
    return o.contiguous(), d.contiguous()


def make_case(variant, H, B, P, S, V=8, seed=0, unnormalised=False, hierarchical=True, clamp="softplus", noise=0.3, white_back=True,
              last_back=False, outside_ray=False):
    """A generator of `variant`, its inputs, P random rays per image and the four draws (CPU tensors).  outside_ray: ray 0 of image 0
    starts at (0.9, 0.9, 0.9) and points away from the volume -- every sample beyond the lookup's clamp on every axis."""
    from cnerf_amd.generators import ImplicitGenerator3d
    from cnerf_amd.generators.siren import FIELD_SPECS
    torch.manual_seed(seed)
    lv = level_shapes(variant, V)
    Z = 32
    c_in = sum(c for c, _ in lv)
    if variant in ("TALLSIREN", "SHORTSIREN"):
        gen = ImplicitGenerator3d(variant, 32, 3, 4, H)
    else:
        gen = ImplicitGenerator3d(variant, Z if FIELD_SPECS[variant].has_global else c_in, c_in, 4, H)
    with torch.no_grad():
        gen.siren.final_layer.weight[3] *= 20
    has_glob = variant == "SHORTSIREN" or (variant != "TALLSIREN" and FIELD_SPECS[variant].has_global)
    vols = [torch.randn(B, c, e, e, e) * 0.5 for c, e in lv]
    glob = torch.randn(B, Z) if has_glob else None
    origins, dirs = random_rays(B, P, seed + 1, unnormalised)
    if outside_ray:
        origins[0, 0] = torch.tensor([0.9, 0.9, 0.9])
        dirs[0, 0] = torch.tensor([1.0, 1.0, 1.0]) / 3 ** 0.5
    n = 2 * S if hierarchical else S
    rng = {"u_strat": torch.rand(B, P, S), "eps_coarse": torch.randn(B, P, S), "u_fine": torch.rand(B, P, S), "eps_final": torch.randn(B, P, n)}
    if not hierarchical:
        del rng["eps_coarse"], rng["u_fine"]
    return SimpleNamespace(variant=variant, gen=gen, vols=vols, glob=glob, origins=origins, dirs=dirs, rng=rng, B=B, P=P, S=S, H=H,
                           hierarchical=hierarchical, clamp=clamp, noise=noise, white_back=white_back, last_back=last_back)


def generator_z(case, vols, glob):
    """z as ImplicitGenerator3d.forward / render_rays take it."""
    if case.variant == "SHORTSIREN":
        return glob
    fv = vols if len(vols) > 1 else vols[0]
    return (fv, glob) if glob is not None else fv


def oracle_run(case, dt=torch.float32, forced_fine_z=None, grads_for=None):
    """The ray oracle on `case`.  grads_for = (w_p (B,P,3), v (B,P)): also the gradients of sum(w_p * pixels) + sum(v * dist) w.r.t. every
    parameter, volume level, the global feature, origins and dirs, as {name: float64 array}.  -> (pixels, dist, aux[, grads])"""
    c = lambda t: t.detach().clone().to(dt)
    req = grads_for is not None
    params = {k: c(v).requires_grad_(req) for k, v in case.gen.siren.state_dict().items()}
    vols = [c(v).requires_grad_(req) for v in case.vols]
    glob = c(case.glob).requires_grad_(req) if case.glob is not None else None
    o, d = c(case.origins).requires_grad_(req), c(case.dirs).requires_grad_(req)
    r = case.rng
    with torch.set_grad_enabled(req):
        px, dist, aux = ray_oracle(oracle_field(case.variant, params, vols, glob, dt), o, d, case.S, RAY_START, RAY_END, case.hierarchical, case.clamp,
                                   case.noise, case.white_back, case.last_back, r["u_strat"], r.get("u_fine"), r.get("eps_coarse"), r.get("eps_final"),
                                   forced_fine_z, dt)
    if not req:
        return px, dist, aux
    wp, v = grads_for
    loss = (px * wp.to(dt)).sum() + (dist * v.to(dt)).sum()
    leaves = list(params.values()) + vols + ([glob] if glob is not None else []) + [o, d]
    names = list(params.keys()) + [f"volume{i}" for i in range(len(vols))] + (["global_feature"] if glob is not None else []) + ["origins", "dirs"]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    out = {k: (g if g is not None else torch.zeros_like(t)).double().numpy() for k, g, t in zip(names, grads, leaves)}
    return px.detach(), dist.detach(), aux, out


def in_band_share(cdf, u, band=2e-6):
    """Share of the draws u (..., S) that lie within `band` of an entry of cdf (..., S-1)."""
    cdf, u = np.asarray(cdf, np.float64), np.asarray(u, np.float64)
    return float(1.0 - (np.abs(u[..., :, None] - cdf[..., None, :]) > band).all(-1).mean())


def cdf_conditioning(case, ref_aux):
    """scaled_err of the oracle's own float32 cdf against its float64 evaluation from the SAME coarse rgb_sigma, depths and draws: what the
    last bit of exp() and of the sums does to this case's cdf.  A ray without density (relu clamp) leaves its cdf to the 2e-5 epsilons
    of sample_pdf, and the reference's own float32 cdf is then 1e-6 .. 5e-6 from exact (measured: TALLSIREN / SHORTSIREN_FRes, 100 rays,
    relu): a case must stay well below a gate it is to carry."""
    from conftest import scaled_err
    z, rs, r = ref_aux["coarse_z"], ref_aux["coarse_rgb_sigma"].detach().float(), case.rng
    _, _, w32 = O.composite(rs, z, r["eps_coarse"], case.noise, case.clamp)
    c32 = O.importance_depths(z, w32, r["u_fine"])[2]
    keep = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        _, _, w64 = O.composite(rs.double(), z.double(), r["eps_coarse"].double(), case.noise, case.clamp)
        c64 = O.importance_depths(z.double(), w64, r["u_fine"].double())[2]
    finally:
        torch.set_default_dtype(keep)
    return scaled_err(c32.numpy(), c64.numpy())


# ---------------------------------------------------------------------------------------------------------------------
# the arithmetic of the header in NumPy float32 (geometry tests)
# ---------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def linspace32(start, end, steps):
    """torch.linspace in float32 as ATen computes it: symmetric halves, fused."""
    start, end = np.float32(start), np.float32(end)
    step = np.float32((end - start) / np.float32(steps - 1))
    i = np.arange(steps)
    lo = _fma32(step, i.astype(np.float32), start)
    hi = _fma32(-step, (steps - 1 - i).astype(np.float32), end)
    return np.where(i < steps // 2, lo, hi).astype(np.float32)


def numpy_geometry(origins, dirs, u, S, ray_start, ray_end):
    """(coarse_z (B,P,S), coarse_points (B,P,S,3)) in float32 from float32 arrays."""
    zl = linspace32(ray_start, ray_end, S)
    z = (zl[None, None, :] + ((u.astype(np.float32) - np.float32(0.5)) * np.float32(zl[1] - zl[0])).astype(np.float32)).astype(np.float32)
    return z, numpy_points(origins, dirs, z)


def numpy_points(origins, dirs, z):
    prod = (dirs.astype(np.float32)[:, :, None, :] * z.astype(np.float32)[..., None]).astype(np.float32)
    return (origins.astype(np.float32)[:, :, None, :] + prod).astype(np.float32)
