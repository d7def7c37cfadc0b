"""GPU stage tests of the per-ray kernels (csrc/ray_kernels.hip) on synthetic inputs, no field network in the loop: the merge +
composite backward, the composite and the inverse-CDF resampling, each against oracle.render_oracle run in float64.  Run on an
MI355X with  pytest -m gpu.

The inputs are built to hit what the golden fixtures never hold: every 64-sample chunk count of a ray and both sides of every
chunk edge, opaque samples (alpha == 1, the shifted transmittance factor 1e-10), densities far below zero and beyond softplus'
linear threshold, tied depths, all-zero and one-hot weights, and draws that sit exactly on a cdf entry.  Every test prints the
figures it gates on before it asserts.
"""
import numpy as np
import pytest
import torch

from conftest import scaled_err
from oracle.checks import bin_mass, flips_outside_band

pytestmark = pytest.mark.gpu

FOV, RAY_START, RAY_END = 49.13, 0.25, 1.95
B_, R_ = 2, 3                      # nine rays per image: three blocks of four waves per image, the last with one live wave
NEG_RAY = (B_ - 1, 4)              # the ray whose densities are all far below zero


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


class _default_dtype:
    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        self.keep = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.keep)


def _plant_ties(z, n):
    """Every seventh depth of a ray copied from its neighbour (a sorted row stays sorted)."""
    idx = torch.arange(6, n, 7)
    z[..., idx] = z[..., idx - 1]


def _rgb_sigma(gen, shape, opaque):
    """rgb ~ N(0,1); sigma ~ 20 N(0,1): relu sees many negatives, softplus arguments beyond its linear threshold of 20; `opaque`: one
    planted sample and ~3 % of the rest at 1e4 (alpha == 1, shifted == 1e-10)."""
    rs = torch.randn(*shape, 4, generator=gen)
    rs[..., 3] *= 20
    if opaque:
        sig = rs[..., 3]
        sig[torch.rand(*shape, generator=gen) < 0.03] = 1e4
        sig[(0,) * (len(shape) - 1) + (shape[-1] // 2,)] = 1e4
    return rs


# ---------------------------------------------------------------------------------------------------------------------------------
# A1  cnerf_merge_composite_backward
# ---------------------------------------------------------------------------------------------------------------------------------
def merge_composite_inputs(S, hier, noise, ties, seed, neg_ray):
    """coarse depths sorted uniform in [0.25, 1.95]; fine depths unordered and concentrated in [1.0, 1.05]; ties (if asked for) inside
    the fine set only; neg_ray: one ray with every density far below zero (no gradient at all under relu; see A1_CASES for softplus);
    independent random upstream gradients."""
    gen = torch.Generator().manual_seed(seed)
    P = R_ * R_
    n = 2 * S if hier else S
    c_z = torch.sort(RAY_START + (RAY_END - RAY_START) * torch.rand(B_, P, S, generator=gen), -1).values
    f_z = 1.0 + 0.05 * torch.rand(B_, P, S, generator=gen)
    if ties:
        _plant_ties(f_z, S)
    c_rs, f_rs = _rgb_sigma(gen, (B_, P, S), True), _rgb_sigma(gen, (B_, P, S), False)
    for rs in (c_rs, f_rs) if neg_ray else ():
        rs[NEG_RAY[0], NEG_RAY[1], :, 3] = -rs[NEG_RAY[0], NEG_RAY[1], :, 3].abs() - 5.0      # no 0.3 * N(0,1) draw lifts it above zero
    eps = torch.randn(B_, P, n, generator=gen) if noise != 0 else None
    gp, gd = torch.randn(B_, 3, R_, R_, generator=gen), torch.randn(B_, R_, R_, generator=gen)
    if hier:
        assert not (f_z.unsqueeze(-1) == c_z.unsqueeze(-2)).any()                              # never fine == coarse
    return dict(c_rs=c_rs, c_z=c_z, f_rs=f_rs if hier else None, f_z=f_z if hier else None, eps=eps, gp=gp, gd=gd)


def merge_composite_grads_oracle(dtype, t, noise, clamp, white, last):
    """d loss / d (coarse, fine) rgb_sigma by autograd through the oracle's merge (stable: ties keep their order in cat[fine, coarse],
    the kernel's rule) and composite in `dtype`; loss = (pixels * gp).sum() + (depth * gd).sum()."""
    from oracle import render_oracle as O
    c = lambda x: None if x is None else x.detach().to(dtype)
    with _default_dtype(dtype):
        cr = c(t["c_rs"]).requires_grad_(True)
        leaves = [cr]
        if t["f_rs"] is not None:
            fr = c(t["f_rs"]).requires_grad_(True)
            leaves.append(fr)
            all_out, all_z, _ = O.merge_by_depth(fr, cr, c(t["f_z"]), c(t["c_z"]), stable=True)
        else:
            all_out, all_z = cr, c(t["c_z"])
        rgb, dist, _ = O.composite(all_out, all_z, c(t["eps"]), noise, clamp, white, last)
        P = R_ * R_
        pixels = rgb.reshape(B_, R_, R_, 3).permute(0, 3, 1, 2) * 2 - 1
        depth = (O.camera_ray_dirs(R_, FOV)[:, 2].reshape(1, P) * dist).reshape(B_, R_, R_)
        loss = (pixels * c(t["gp"])).sum()
        if t["gd"] is not None:
            loss = loss + (depth * c(t["gd"])).sum()
        grads = torch.autograd.grad(loss, leaves)
    return [g.double().numpy() for g in grads]


# neg: the ray without density is planted.  Every relu case has it (no gradient at all there).  Under softplus such a ray has alphas of
# ~1e-6 = 1 - exp(-x) with x next to fp32's resolution of 1, so the float32 oracle itself is percent-level off on it: two softplus cases
# keep it and gate it on its own, against its own floor, outside the 1e-4 guard of the reference floor (which covers all other rays).
#        S  hier  clamp       white  last   noise ties  upstream  neg
A1_CASES = [
    (2, True, "relu", False, False, 0.0, False, "both", True),
    (3, True, "softplus", True, False, 0.3, False, "both", False),
    (32, True, "relu", True, True, 0.3, False, "both", True),
    (33, True, "softplus", False, True, 0.0, True, "both", False),
    (64, True, "relu", True, False, 0.3, False, "both", True),
    (65, True, "softplus", True, True, 0.3, False, "both", True),
    (65, True, "relu", True, True, 0.3, False, "no_depth", True),          # grad_depth = NULL
    (97, True, "relu", False, True, 0.0, False, "both", True),
    (97, True, "softplus", True, False, 0.3, False, "no_pixels", False),   # grad_pixels = 0
    (128, True, "softplus", False, False, 0.3, True, "both", True),
    (128, True, "relu", True, True, 0.3, False, "both", True),
    (2, False, "relu", True, True, 0.3, False, "both", True),
    (65, False, "softplus", True, False, 0.0, False, "both", False),
    (128, False, "relu", False, True, 0.3, False, "both", True),
]


def a1_case(case):
    """(inputs, float64 gradients, float32 gradients) of one A1 case; host only."""
    S, hier, clamp, white, last, noise, ties, upstream, neg = case
    t = merge_composite_inputs(S, hier, noise, ties, seed=1000 + 7 * S + (1 if hier else 0) + (2 if clamp == "relu" else 0), neg_ray=neg)
    if upstream == "no_depth":
        t["gd"] = None
    elif upstream == "no_pixels":
        t["gp"] = torch.zeros_like(t["gp"])
    exact = merge_composite_grads_oracle(torch.float64, t, noise, clamp, white, last)
    ref32 = merge_composite_grads_oracle(torch.float32, t, noise, clamp, white, last)
    return t, exact, ref32


@pytest.mark.parametrize("case", A1_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_merge_composite_backward_vs_float64_autograd(dev, case):
    """cnerf_merge_composite_backward on its own against float64 autograd through the oracle's merge + composite, with independent
    random upstream gradients for every pixel and every ray's depth (so the addressing of grad_pixels + b*3*P + p and grad_depth[ray],
    the dz factor and the grad_depth == NULL branch all count), at n = 4 .. 256 merged samples: every chunk count of the 64-lane
    scans, sample n-1 in every chunk, the suffix sum carried across up to four chunks.  Two images of nine rays.  Planted: opaque
    coarse samples, densities beyond +-20, fine depths concentrated in 5 % of the ray and (two cases) tied, one ray with no density.
    Gate per output tensor, colour and density columns apart:  scaled_err(hip, fp64) < max(1e-5, 2.5 x scaled_err(fp32 oracle, fp64)),
    and the fp32 oracle itself within 1e-4 of float64 so that the gate cannot drift loose.

    Measured on an MI355X, maximum over the cases, kernel vs float64 | fp32 oracle vs float64 (the floor):
        coarse colour 1.5e-6 | 5.0e-6      coarse density 2.8e-6 | 2.8e-6
        fine colour   2.6e-5 | 2.4e-5      fine density   2.9e-6 | 3.2e-6
    so the colour and density gates of the coarse samples and the fine density rest on the constant 1e-5 (margin 3x or more), the fine
    colour gate on 2.5 x floor (the kernel sits at 1.0-1.3 x the floor in every case).  Every case finite, the opaque samples at 1e4
    included.  The no-density ray of the two softplus cases, gated on its own: fine colour 3.7e-2 | 3.7e-2 (S = 65) and 2.0e-2 | 1.3e-2
    (S = 128) -- percent-level in the fp32 oracle and the kernel alike, i.e. those rows are effectively not gated, see A1_CASES -- while
    its coarse colour 4.5e-7 | 3.8e-7, coarse density 6.9e-7 | 6.6e-7 and fine density 5.5e-7 | 6.5e-7 stay on the 1e-5 term.
    The test prints these figures per case ("A1 ..." lines, pytest -s)."""
    from cnerf_amd import ops
    from cnerf_amd.generators import ImplicitGenerator3d
    S, hier, clamp, white, last, noise, ties, upstream, neg = case
    t, exact, ref32 = a1_case(case)
    net = ImplicitGenerator3d("SHORTSIREN_FG", 32, 32, 4, 64).siren
    cfg = ops.make_cfg(net, B_, 8, R_, S, FOV, RAY_START, RAY_END, noise, hier, white, last, clamp)
    G = lambda x: None if x is None else x.to(dev)
    gc, gf = ops.merge_composite_backward(cfg, G(t["c_rs"]), G(t["c_z"]), G(t["f_rs"]), G(t["f_z"]), G(t["eps"]), G(t["gp"]), G(t["gd"]))
    torch.cuda.synchronize()
    assert (gf is not None) == hier
    failures = []
    for nm, got, ex, r32 in zip(("coarse", "fine"), (gc, gf), exact, ref32):
        got = got.cpu().numpy()
        assert np.isfinite(got).all(), nm
        # the softplus cases that keep the ray without density: that ray apart, against its own floor and outside the floor's guard
        flat = lambda a: a.reshape(B_ * R_ * R_, S, 4)
        i_neg = NEG_RAY[0] * R_ * R_ + NEG_RAY[1]
        if neg and clamp == "softplus":
            rest = np.arange(B_ * R_ * R_) != i_neg
            views = [("", lambda a: flat(a)[rest], True), (" no-density ray", lambda a: flat(a)[i_neg], False)]
        else:
            views = [("", flat, True)]
        for what, view, guarded in views:
            for col, sl in (("rgb", np.s_[..., :3]), ("sigma", np.s_[..., 3])):
                g_, e_, r_ = view(got)[sl], view(ex)[sl], view(r32)[sl]
                floor, err = scaled_err(r_, e_), scaled_err(g_, e_)
                print(f"A1 {case} {nm} {col}{what}: hip_vs_fp64 {err:.3e} ref32_vs_fp64 {floor:.3e}")
                if guarded and not floor < 1e-4:
                    failures.append((nm, col, "reference floor", floor))
                if not err < max(1e-5, 2.5 * floor):
                    bad = np.argwhere(np.abs(g_ - e_) == np.abs(g_ - e_).max())[0]
                    failures.append((nm, col + what, err, floor, "worst at", tuple(int(i) for i in bad)))
        # rows of dead samples are exactly what autograd gives: the ray without density gets no density gradient under relu, and its
        # colour rows carry the weights 0 (1 on the last sample with last_back) exactly.  (Equal by construction, not by luck: every
        # factor is 0 or 1 there and 2 * grad_pixels is exact in fp32; a failure here after a compiler change means a product with 0 was
        # reordered into something that is not 0, e.g. inf * 0.)
        if clamp == "relu":
            assert np.array_equal(got[NEG_RAY], ex[NEG_RAY].astype(np.float32)), nm
            sig = (t["c_rs"] if nm == "coarse" else t["f_rs"])[..., 3].numpy()
            dead = sig < -10.0                                         # beyond any 0.3 * N(0,1) draw
            assert (got[..., 3][dead] == 0).all() and (ex[..., 3][dead] == 0).all(), nm
    assert not failures, failures


# ---------------------------------------------------------------------------------------------------------------------------------
# A2  cnerf_composite
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 63, 64, 65, 128, 129, 255, 256])
def test_composite_vs_float64(dev, n):
    """cnerf_composite on nine rays of n samples, both sides of every 64-sample chunk edge up to MAX_N = 256, every combination of
    clamp mode, white_back and last_back, with injected noise and without: weights, colour and distance within 1e-5 (scaled_err) of
    the oracle's composite in float64; the weights sum to at most 1 + 1e-5, and to 1 within 1e-6 with last_back.  Planted: opaque
    samples, densities beyond +-20, tied depths (delta == 0), one ray with no density (its weights are exactly 0 under relu).

    Measured on an MI355X, maximum over n and the flags, kernel vs float64: weights 1.5e-6, colour 7.0e-7, distance 8.5e-7 (gate 1e-5);
    sum(w) - 1 at most 4.2e-8.  For scale: the oracle's own float32 composite is 3.4e-6 (weights, n = 256), 7.6e-7 (colour) and 6.2e-7
    (distance) from float64 on these inputs.  The test prints the figures per flag combination ("A2 ..." lines, pytest -s)."""
    from cnerf_amd import ops
    from oracle import render_oracle as O
    gen = torch.Generator().manual_seed(2000 + n)
    rays = 9
    z = torch.sort(RAY_START + (RAY_END - RAY_START) * torch.rand(rays, n, generator=gen), -1).values
    if n >= 8:
        _plant_ties(z, n)
    rs = _rgb_sigma(gen, (rays, n), True)
    rs[4, :, 3] = -rs[4, :, 3].abs() - 5.0
    eps_t = torch.randn(rays, n, generator=gen)
    worst = {}
    for clamp in ("relu", "softplus"):
        for white in (False, True):
            for last in (False, True):
                for eps in (eps_t, None):
                    with _default_dtype(torch.float64):
                        rgb64, dist64, w64 = (x[0].numpy() for x in O.composite(rs.double()[None], z.double()[None],
                                                                                None if eps is None else eps.double()[None], 0.3, clamp, white, last))
                    rgb, dist, w = (x.cpu().numpy() for x in ops.composite(rs.to(dev), z.to(dev), None if eps is None else eps.to(dev), 0.3, clamp, white, last))
                    tag = (clamp, white, last, eps is not None)
                    e = {"weights": scaled_err(w, w64), "rgb": scaled_err(rgb, rgb64), "dist": scaled_err(dist, dist64)}
                    wsum = w.astype(np.float64).sum(-1)
                    print(f"A2 n={n} {tag}: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()) + f" max sum(w) - 1 {wsum.max() - 1:.3e}")
                    for k, v in e.items():
                        worst[k] = max(worst.get(k, 0.0), v)
                    assert np.isfinite(w).all() and np.isfinite(rgb).all() and np.isfinite(dist).all(), tag
                    assert e["weights"] < 1e-5 and e["rgb"] < 1e-5 and e["dist"] < 1e-5, (tag, e)
                    assert (wsum <= 1 + 1e-5).all(), tag
                    if last:
                        assert np.abs(wsum - 1).max() < 1e-6, (tag, np.abs(wsum - 1).max())
                    if clamp == "relu":
                        assert (w[4, :-1] == 0).all() and w[4, -1] == (1.0 if last else 0.0), tag
    print(f"A2 n={n} worst: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------------------
# A3  cnerf_resample
# ---------------------------------------------------------------------------------------------------------------------------------
def resample_fp32(z, cdf, u):
    """The oracle's inverse-CDF formula (render_oracle.importance_depths) in float32 arithmetic from a GIVEN float32 cdf:
    (fine_z, inds, bin width of every draw)."""
    S = z.shape[1]
    assert z.dtype == cdf.dtype == u.dtype == np.float32
    bins = np.float32(0.5) * (z[:, :-1] + z[:, 1:])
    inds = np.stack([np.searchsorted(c, uu, "left") for c, uu in zip(cdf, u)]).astype(np.int64)
    below, above = np.maximum(inds - 1, 0), np.minimum(inds, S - 2)
    c0, c1 = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
    b0, b1 = np.take_along_axis(bins, below, 1), np.take_along_axis(bins, above, 1)
    den = c1 - c0
    den = np.where(den < np.float32(1e-5), np.float32(1.0), den)
    fine = b0 + (u - c0) / den * (b1 - b0)
    assert fine.dtype == np.float32
    return fine, inds, (b1 - b0).astype(np.float64)


@pytest.mark.parametrize("S", [2, 3, 4, 64, 65, 128])
def test_resample_vs_oracle(dev, S):
    """cnerf_resample on 32 rays: eight each with random weights, all-zero weights, one-hot weights on an interior sample and one-hot
    weights on sample 0 (which the pdf ignores).
    First call, random u plus a planted 0.0 and nextafter(1, 0) per ray, against the oracle in float64: cdf within 1e-6; bin indices
    equal outside a 2e-6 band around the cdf entries (no hard flip, under 1e-3 of the random draws flipped); depths within 1e-5 in
    bins of mass above 1e-2 and within the draw's own bin width everywhere else.
    Second call, u planted ON the kernel's own returned cdf entries and one ulp above and below them (where that stays in [0, 1)):
    the bin index of EVERY draw equals np.searchsorted(cdf, u, 'left') -- the `<` of the binary search and the below / above clamps
    at both ends, independent of any rounding upstream -- and the depth equals the oracle's formula evaluated in float32 from that
    cdf to 1e-6 of the draw's bin width.  That bound is below one fp32 ulp of a depth: it asks for the same fp32 operations in the same
    order as numpy's (the library is built with -ffp-contract=off and correctly rounded division), so equality holds by construction;
    should a compiler change break it, look at contraction and the division before suspecting the kernel's logic.

    Measured on an MI355X, maximum over S, kernel vs float64: cdf 1.1e-7 (gate 1e-6), depths in bins of mass above 1e-2 3.2e-7 (gate
    1e-5), no bin index flipped at all, |depth error| - bin width at most 6e-8; planted draws: no bin index off, depth error / bin width
    0 (bit-equal to the float32 formula).  For scale: the oracle's own float32 cdf is 3.5e-7 from float64 at S = 128 and its depths in
    well-populated bins 2.4e-7.  The test prints the figures ("A3 ..." lines, pytest -s)."""
    from cnerf_amd import ops
    from oracle import render_oracle as O
    gen = torch.Generator().manual_seed(3000 + S)
    rays, per = 32, 8
    z = torch.sort(RAY_START + (RAY_END - RAY_START) * torch.rand(rays, S, generator=gen), -1).values
    w = torch.rand(rays, S, generator=gen)
    w /= w.sum(-1, keepdim=True)
    w[per:] = 0.0
    if S >= 3:
        w[2 * per:3 * per, torch.randint(1, S - 1, (1,), generator=gen).item()] = 1.0
    w[3 * per:, 0] = 1.0
    u = torch.rand(rays, S, generator=gen)
    u[:, 0] = 0.0
    u[:, 1] = float(np.nextafter(np.float32(1), np.float32(0)))
    n_planted = 2

    fine, inds, cdf = (x.cpu().numpy() for x in ops.resample(z.to(dev), w.to(dev), u.to(dev)))
    with _default_dtype(torch.float64):
        fine64, inds64, cdf64 = (x[0].numpy() for x in O.importance_depths(z.double()[None], w.double()[None], u.double()[None]))
    un = u.numpy()
    assert np.isfinite(fine).all() and np.isfinite(cdf).all()
    e_cdf = scaled_err(cdf, cdf64)
    print(f"A3 S={S}: cdf {e_cdf:.3e}")
    assert e_cdf < 1e-6
    if S > n_planted:
        rnd = np.s_[:, n_planted:]
        hard, frac = flips_outside_band(cdf64, un[rnd], inds[rnd], inds64[rnd].astype(np.int32), 2e-6)
        print(f"A3 S={S}: hard flips {hard} flipped fraction {frac:.3e}")
        assert hard == 0 and frac < 1e-3
    same = inds == inds64
    well = same & (bin_mass(cdf64, inds64) > 1e-2)
    if well.any():
        e_well = scaled_err(fine[well], fine64[well])
        print(f"A3 S={S}: depths in bins of mass > 1e-2 {e_well:.3e} ({well.mean():.2f} of the draws)")
        assert e_well < 1e-5
    # everywhere else: inside the draw's bin, or -- a draw whose index flipped inside the band sits on the edge between two bins -- inside
    # the union of the kernel's and the reference's bin (1e-6: rounding of the bin ends themselves)
    bins64 = 0.5 * (z.double().numpy()[:, :-1] + z.double().numpy()[:, 1:])
    ends = lambda i: (np.take_along_axis(bins64, np.maximum(i - 1, 0), 1), np.take_along_axis(bins64, np.minimum(i, S - 2), 1))
    (lo_k, hi_k), (lo_r, hi_r) = ends(inds.astype(np.int64)), ends(inds64.astype(np.int64))
    lo, hi = np.minimum(lo_k, lo_r), np.maximum(hi_k, hi_r)
    over = np.abs(fine - fine64) - (hi - lo)
    print(f"A3 S={S}: max (|depth error| - bin width) {over.max():.3e}, draws with a flipped index {int((~same).sum())}")
    assert (over <= 1e-6).all()
    assert ((fine >= lo - 1e-6) & (fine <= hi + 1e-6)).all()

    # the same rays three times over: u on the cdf entries, one ulp below, one ulp above
    c = np.concatenate([cdf, np.full((rays, 1), 0.5, np.float32)], 1)            # S - 1 entries and one filler draw
    up, down = np.nextafter(c, np.float32(2)), np.nextafter(c, np.float32(-1))
    u2 = np.concatenate([c, down, up], 0)
    u2 = np.where((u2 >= 0) & (u2 < 1), u2, np.float32(0.5)).astype(np.float32)
    z3, w3 = z.repeat(3, 1), w.repeat(3, 1)
    fine2, inds2, cdf2 = (x.cpu().numpy() for x in ops.resample(z3.to(dev), w3.to(dev), torch.from_numpy(u2).to(dev)))
    assert np.array_equal(cdf2, np.tile(cdf, (3, 1)))
    want_fine, want_inds, width2 = resample_fp32(z3.numpy(), cdf2, u2)
    n_bad = int((inds2 != want_inds).sum())
    err2 = np.abs(fine2.astype(np.float64) - want_fine.astype(np.float64))
    rel2 = float((err2 / np.maximum(width2, 1e-30))[err2 > 0].max()) if (err2 > 0).any() else 0.0
    print(f"A3 S={S}: planted draws {u2.size}, bin indices off {n_bad}, max depth error / bin width {rel2:.3e}")
    assert n_bad == 0, np.argwhere(inds2 != want_inds)[:8]
    assert (err2 <= 1e-6 * width2).all(), np.argwhere(err2 > 1e-6 * width2)[:8]
