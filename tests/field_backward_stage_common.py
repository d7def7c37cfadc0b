"""The fp32 field backward stage (cnerf_field_backward / cnerf_field_backward_points) row by row in float64: the formulas of
include/cnerf.h and their rounding bounds, shared by tests/test_gpu_field_backward_stage.py (the kernels) and
tests/test_field_backward_stage_cpu.py (a float32 torch emulation of the stage, honest and corrupted).

Every check is LAYER-LOCAL: the float64 value of a row is computed from the rows the stage itself stored one step earlier (act_feat ->
slab 0 -> slab 1 ...; act_go -> last slab of act_g -> ... -> gradient volume), so no error is amplified through the network and every
element is held to the rounding of ONE step.  u = 2^-24 throughout; dot_bound(k, A, B) = (k + 2) u |A|^T |B| is the bound of a length-k
fp32 dot product summed in any order (tests/test_gpu_pfilm_finish.py).

Derivations
-----------
lookup      ic = ((p / hv + 1) V - 1) / 2 is formed in fp32 from the fp32 position: four roundings, |d ic| <= u (V |g| + 2 V |g + 1| +
            |(g + 1) V - 1|) / 2 <= 3.5 u V wherever the clamp to [0, V - 1] does not remove the error altogether (|g| <= 1 there);
            DELTA = 4 u V per axis.  lo = ic - floor(ic) and hi = floor(ic) + 1 - ic are exact.  The interpolant is continuous and
            piecewise trilinear in ic, with slope <= 2 max |node| along an axis, the nodes being those of the cells within DELTA of the
            float64 coordinate: inside [i0 - 1, i0 + 2] per axis (a coordinate that rounds across an integer changes the cell, never
            the value by more than this).  Weight error: 3 axes * DELTA * 2 * Mnbr = 6 DELTA Mnbr.  Each fp32 weight is two products
            (2 u relative), each addend one product, the 8 addends are summed sequentially: (8 + 2) u + 2 u of sum w |corner|.
                bound(act_feat) = 12 u sum_k w_k |q_k| + 6 DELTA Mnbr
            The xyz tile is a copy: equality, zeros in the padding.
pre         pre = W x + b (a residual fc2: + x_in): k = K + 1 (+ 1) terms, K the REAL input width (adding the exact zeros of a padded
            tile rounds nothing): d pre = dot_bound(k, ...).
arg         arg = fl(fl(freq pre) + phase):  d arg = |freq| d pre + 2 u (|freq pre| + |arg|)   (freq = 1, phase = 0: sine, residual)
sin, cos    |sin'|, |cos'| <= 1: d arg + 1.2e-7 (sine polynomial) / + 1.5e-7 (cosine polynomial), the documented maxima on |x| <= 300
            (csrc/cnerf_dev.hpp); |arg| <= 300 is asserted.  Dropout: the row times keep * s, s = fp32(1 / (1 - p)): the bound times s,
            plus 2 u |value| (s itself and the product are rounded); a dropped element is exactly zero (bound 0).
per-point   m = LeakyReLU(Wm1 feat + bm1): dot_bound(33) * slope (its spare unit is the slope's product).  f = 15 f_raw + 30 with
FiLM        d f = 15 dot_bound(257) + u (|15 f_raw| + |f|); d phase = dot_bound(257); d pre = dot_bound(K + 1), K = 3 for layer 0;
            d arg = |f| d pre + |pre| d f + d f d pre + d phase + 2 u (|f pre| + |arg|).  The stored rows cos f and cos 15 pre are
            products of two computed factors: |a| db + |b| da + da db + u |ab| (15 pre: one more u |15 pre|).
go          upstream * (s (1 - s)): three roundings, 3 u relative; channel 3 (and every channel without the sigmoid) bit-equal.
chain       the transposed product reads fp32 operands the stage stored (act_go; act_g[m] * freq_m rounded to fp32, a single IEEE
            product that float32 NumPy reproduces bit for bit); its result times the stored cosine row:
                bound(act_g) = |cos| dot_bound(k, operand, W) + 2 u |value|,  k = 4 (head), H, or H + 1 (the identity term of a block)
volume      addend = fl(g_feat w_k), g_feat = (act_g[0] freq_0) W_0[:, columns] with d g = dot_bound(H, ...), the fp32 weight with
            absolute error 3 DELTA (three factors <= 1) + 2 u w, the product u:
                bound = scatter(w d g) + (3 + 2 k) u scatter(w |g|) + 3 DELTA scatter_nbr(|g|)
            -- the second term is the reordering of the k atomic addends of a voxel channel (two orders of k addends differ by
            <= 2 (k - 1) u sum |addend|); k <= 8 n_per_image, and no more than the points whose 4^3 neighbourhood holds the voxel,
            which is what is used; scatter_nbr spreads over the 4^3 voxels a coordinate within DELTA of the float64 one can touch.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from test_gpu_pfilm_finish import U, dot_bound, within

SIN_POLY, COS_POLY = 1.2e-7, 1.5e-7        # csrc/cnerf_dev.hpp: sin_pi_reduced / sincos_pi_reduced on |x| <= 300
ARG_MAX = 300.0
HALF_VOXEL = float(np.float32(1.2) / np.float32(2.0))      # cfg.voxel_length / 2.0f as the kernels form it
F64 = np.float64


@dataclass
class Matrix:
    """One activation slab's matrix: W (H, K real), b (H); film: index of its FiLM vectors or None; role plain | fc1 | fc2;
    drop: index of its dropout layer (None: a residual block has none)."""
    W: np.ndarray
    b: np.ndarray
    film: Optional[int]
    role: str
    drop: Optional[int]


@dataclass
class StageNet:
    kinds: Tuple[str, ...]
    H: int
    sigmoid: bool
    input: str                              # feat | feat_xyz | pyramid | position | xyz (per-point FiLM)
    mats: List[Matrix]
    head_W: np.ndarray                      # (4, H)
    head_b: np.ndarray
    map: Optional[Tuple[np.ndarray, ...]] = None       # per-point FiLM: Wm1 (256, 32), bm1, Wm2 (2 L H, 256), bm2

    @property
    def pfilm(self):
        return self.kinds[0] == "pfilm"

    @property
    def n_film(self):
        return sum(k == "film" for k in self.kinds)


def stage_net(net):
    """StageNet (float32 arrays) of a cnerf_amd.generators.siren module."""
    a = lambda p: p.detach().cpu().numpy().astype(np.float32)
    mats, films, drops = [], 0, 0
    for kind, blk in zip(net.spec.layers, net.network):
        if kind == "res":
            mats += [Matrix(a(blk.fc1.weight), a(blk.fc1.bias), None, "fc1", None), Matrix(a(blk.fc2.weight), a(blk.fc2.bias), None, "fc2", None)]
        else:
            mats.append(Matrix(a(blk.layer.weight), a(blk.layer.bias), films if kind == "film" else None, "plain", drops))
            films += kind == "film"
            drops += 1
    mp = None
    if net.spec.input == "xyz":
        seq = net.mapping_network.network
        mp = (a(seq[0].weight), a(seq[0].bias), a(seq[2].weight), a(seq[2].bias))
    return StageNet(tuple(net.spec.layers), int(net.hidden_dim), bool(net.spec.sigmoid_rgb), net.spec.input, mats, a(net.final_layer.weight),
                    a(net.final_layer.bias), mp)


@dataclass
class StageCase:
    """Inputs of one stage call, restricted to the images of the chunk: levels (n_images, V, V, V, C) channel-last, freq / phase
    (n_images, n_film H) or None, points / upstream / saved (n_images, npi, 3 | 4), drop = (p, keep (n_drop, n_images, npi, H)) or None."""
    levels: List[np.ndarray]
    freq: Optional[np.ndarray]
    phase: Optional[np.ndarray]
    points: np.ndarray
    upstream: np.ndarray
    saved: np.ndarray
    drop: Optional[Tuple[float, np.ndarray]] = None


def input_tiles(sn, levels):
    """[(level or -1 for the xyz tile, first channel)] of layer 0's 32-wide input tiles, in act_feat's column order."""
    tiles = [(i, c) for i, v in enumerate(levels) for c in range(0, v.shape[-1], 32)]
    if sn.pfilm:
        return tiles
    return tiles + ([(-1, 0)] if sn.input in ("feat_xyz", "position") else [])


def act_sizes(sn, n, levels):
    """Floats of (act_feat, act_h, act_c, act_g, act_go) for n rows, as include/cnerf.h sizes them."""
    H, L = sn.H, len(sn.kinds)
    if sn.pfilm:
        return 32 * n, L * n * H + 256 * n, 3 * L * n * H, 3 * L * n * H, 4 * n
    S = len(sn.mats)
    return 32 * len(input_tiles(sn, levels)) * n, S * n * H, S * n * H, S * n * H, 4 * n


# ---- trilinear geometry in float64 from the float32 positions (oracle.trilinear_corners' conventions) ---------------------------------
def corners64(points, V):
    """i0 (n, 3) int64 in x, y, z order, lo, hi (n, 3) float64."""
    ic = np.clip(((points.astype(F64) / HALF_VOXEL + 1.0) * V - 1.0) / 2.0, 0.0, V - 1.0)
    i0 = np.floor(ic)
    return i0.astype(np.int64), ic - i0, (i0 + 1.0) - ic


def corner_list(points, V):
    """The 8 corners in ATen's order (x fastest): [(voxel index (n,), weight (n,))], indices clamped (a clamped corner has weight 0)."""
    i0, lo, hi = corners64(points, V)
    out = []
    for k in range(8):
        d = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
        idx = np.minimum(i0 + d, V - 1)
        w = np.where(d == 1, lo, hi).prod(axis=1)
        out.append(((idx[:, 2] * V + idx[:, 1]) * V + idx[:, 0], w))
    return out


def nbr_max(vol):
    """max |vol| over the 4^3 nodes [i - 1, i + 2] per axis (clamped into the volume) around every node i: vol (B, V, V, V, C)."""
    V = vol.shape[1]
    pad = np.pad(np.abs(vol), ((0, 0), (1, 2), (1, 2), (1, 2), (0, 0)), mode="edge")
    out = np.zeros(vol.shape, vol.dtype)
    for oz in range(4):
        for oy in range(4):
            for ox in range(4):
                np.maximum(out, pad[:, oz:oz + V, oy:oy + V, ox:ox + V], out=out)
    return out


def nbr_spread(acc):
    """acc (B, V, V, V, C) holds one value per cell i0: every node of [i0 - 1, i0 + 2] per axis (clamped) receives it."""
    V = acc.shape[1]
    M = np.zeros((V, V))
    for o in range(-1, 3):
        np.add.at(M, (np.clip(np.arange(V) + o, 0, V - 1), np.arange(V)), 1.0)
    return np.einsum("az,by,cx,nzyxk->nabck", M, M, M, acc, optimize=True)


def _delta(V):
    return 4.0 * U * V


def lookup64(vol, points, cc):
    """Channels [cc, cc + 32) of vol (n_images, V, V, V, C) at points (n_images, npi, 3): value and bound, (n, 32) each."""
    B, V = vol.shape[0], vol.shape[1]
    npi = points.shape[1]
    pts = points.reshape(-1, 3)
    flat = vol.reshape(B * V ** 3, -1)[:, cc:cc + 32]
    img = np.repeat(np.arange(B), npi) * V ** 3
    want, absum = np.zeros((B * npi, 32)), np.zeros((B * npi, 32))
    for idx, w in corner_list(pts, V):
        q = flat[img + idx].astype(F64)
        want += w[:, None] * q
        absum += w[:, None] * np.abs(q)
    i0 = corners64(pts, V)[0]
    mnbr = nbr_max(vol[..., cc:cc + 32]).reshape(B * V ** 3, 32)[img + (i0[:, 2] * V + i0[:, 1]) * V + i0[:, 0]].astype(F64)
    return want, 12.0 * U * absum + 6.0 * _delta(V) * mnbr


def scatter64(gfeat, dg, points, V, npi_bound):
    """float64 scatter of gfeat (n_images, npi, 32) with the trilinear weights: value and bound, (n_images, V, V, V, 32)."""
    B, npi = points.shape[0], points.shape[1]
    pts = points.reshape(-1, 3)
    img = torch.from_numpy(np.repeat(np.arange(B), npi) * V ** 3)
    g, ag, dg = (torch.from_numpy(np.ascontiguousarray(t.reshape(-1, 32), dtype=F64)) for t in (gfeat, np.abs(gfeat), dg))
    want, carried, absum, cell, count = (torch.zeros((B * V ** 3, 32), dtype=torch.float64) for _ in range(5))
    for idx, w in corner_list(pts, V):
        i, w = img + torch.from_numpy(idx), torch.from_numpy(w)[:, None]
        want.index_add_(0, i, w * g)
        carried.index_add_(0, i, w * dg)
        absum.index_add_(0, i, w * ag)
    i0 = corners64(pts, V)[0]
    i = img + torch.from_numpy((i0[:, 2] * V + i0[:, 1]) * V + i0[:, 0])
    cell.index_add_(0, i, ag)
    count.index_add_(0, i, torch.ones_like(ag))
    nbr = nbr_spread(cell.numpy().reshape(B, V, V, V, 32)).reshape(B * V ** 3, 32)
    # addends a voxel channel can receive: one per point whose 4^3 neighbourhood holds the voxel, at most 8 per point of the image
    k = np.minimum(nbr_spread(count.numpy().reshape(B, V, V, V, 32)).reshape(B * V ** 3, 32), 8.0 * npi_bound)
    bound = carried.numpy() + (3 + 2 * k) * U * absum.numpy() + 3.0 * _delta(V) * nbr
    want, bound = want.numpy(), bound
    return want.reshape(B, V, V, V, 32), bound.reshape(B, V, V, V, 32)


# ---- the rows ---------------------------------------------------------------------------------------------------------------------------
def _film_rows(t, film, H, npi):
    """(n, H) rows of FiLM vector `film` of t (n_images, n_film H): every point of an image sees its image's vector."""
    return np.repeat(t[:, film * H:(film + 1) * H].astype(F64), npi, axis=0)


def _keep_rows(case, d, n, H):
    """(factor (n, H), s) of dropout layer d: keep * s, s = fp32(1 / (1 - p)) as the host forms it; (1, 1) without dropout."""
    if case.drop is None or d is None:
        return None, 1.0
    p, keep = case.drop
    s = float(np.float32(1.0) / np.float32(1.0 - float(np.float32(p))))
    return keep[d].reshape(n, H).astype(F64) * s, s


def _dropped(want, bound, factor, s):
    if factor is None:
        return want, bound
    return want * factor, (factor != 0) * (s * bound + 2 * U * abs(want * factor))


def _prod_bound(a, da, b, db):
    return np.abs(a) * db + np.abs(b) * da + da * db + U * np.abs(a * b)


class StageRows:
    """The chunk buffers of one call as float64 views."""

    def __init__(self, sn, case, out):
        self.sn, self.case = sn, case
        B, npi = case.points.shape[0], case.points.shape[1]
        self.B, self.npi, self.n, H = B, npi, B * npi, sn.H
        n, L = self.n, len(sn.kinds)
        sizes = act_sizes(sn, n, case.levels)
        flat = {k: np.asarray(out[k], np.float32).reshape(-1) for k in ("act_feat", "act_h", "act_c", "act_g", "act_go")}
        for k, want in zip(flat, sizes):
            assert flat[k].size == want, (k, flat[k].size, want)
            assert np.isfinite(flat[k]).all(), k
        self.feat = flat["act_feat"].reshape(n, -1)
        self.go = flat["act_go"].reshape(n, 4)
        if sn.pfilm:
            self.h = flat["act_h"][:L * n * H].reshape(L, n, H)
            self.m = flat["act_h"][L * n * H:].reshape(n, 256)
            self.c = flat["act_c"].reshape(3 * L, n, H)
            self.g = flat["act_g"][:L * n * H].reshape(L, n, H)
            self.G = flat["act_g"][L * n * H:].reshape(n, 2 * L * H)
        else:
            S = len(sn.mats)
            self.h, self.c, self.g = (flat[k].reshape(S, n, H) for k in ("act_h", "act_c", "act_g"))
        self.grad_vols = [np.asarray(v, np.float32) for v in out.get("grad_vols", [])]


def check_forward_rows(sn, case, out, tag=""):
    """act_feat, act_h, act_c (and m) of the fp32 STORE forward, each layer from the stage's own stored input of that layer."""
    r = StageRows(sn, case, out)
    n, H, npi = r.n, sn.H, r.npi
    pts = case.points.reshape(n, 3)
    # layer 0's input tiles
    for tk, (lvl, cc) in enumerate(input_tiles(sn, case.levels)):
        got = r.feat[:, 32 * tk:32 * tk + 32]
        if lvl < 0:
            want = np.zeros((n, 32))
            want[:, :3] = pts
            within(got, want, np.zeros((n, 32)), f"{tag}act_feat xyz tile")
        else:
            want, bound = lookup64(case.levels[lvl], case.points, cc)
            within(got, want, bound, f"{tag}act_feat level {lvl} ch {cc}")
    if sn.pfilm:
        return _check_forward_pfilm(sn, case, r, tag)
    k0 = sn.mats[0].W.shape[1]
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=F64))       # (float64 torch: the same arithmetic on every core)
    for s, mt in enumerate(sn.mats):
        if s == 0:
            x = t64(r.feat[:, :k0])                 # the real columns: features (|| xyz), or xyz alone; the padding is checked above
            k = k0 + 1
        else:
            x, k = t64(r.h[s - 1]), H + 1
        W, b = t64(mt.W), t64(mt.b)
        pre = x @ W.T + b
        absum = x.abs() @ W.abs().T + b.abs()
        if mt.role == "fc2":                                           # pre = x_in + W2 y + b2: x_in is the slab in front of fc1
            xin = t64(r.h[s - 2])
            pre, absum, k = pre + xin, absum + xin.abs(), k + 1
        dpre = (k + 2) * U * absum
        if mt.film is not None:
            fr, ph = t64(_film_rows(case.freq, mt.film, H, npi)), t64(_film_rows(case.phase, mt.film, H, npi))
            arg = fr * pre + ph
            darg = fr.abs() * dpre + 2 * U * ((fr * pre).abs() + arg.abs())
        else:                                                          # freq = 1, phase = 0
            arg = pre
            darg = dpre + 4 * U * arg.abs()
        assert float(arg.abs().max()) <= ARG_MAX, (s, float(arg.abs().max()))
        factor, sc = _keep_rows(case, mt.drop, n, H)
        factor = None if factor is None else t64(factor)
        within(r.h[s], *_dropped(torch.sin(arg), darg + SIN_POLY, factor, sc), f"{tag}act_h[{s}] {mt.role}")
        within(r.c[s], *_dropped(torch.cos(arg), darg + COS_POLY, factor, sc), f"{tag}act_c[{s}] {mt.role}")


def _check_forward_pfilm(sn, case, r, tag):
    n, H, L = r.n, sn.H, len(sn.kinds)
    Wm1, bm1, Wm2, bm2 = (t.astype(F64) for t in sn.map)
    feat = r.feat.astype(F64)
    mpre = feat @ Wm1.T + bm1
    slope = np.where(mpre > 0, 1.0, float(np.float32(0.2)))
    # (an element whose float64 sign differs from the kernel's lies within its own bound of zero on both sides)
    dm = dot_bound(33, feat.T, Wm1.T) + 35 * U * np.abs(bm1)
    within(r.m, mpre * slope, np.maximum(dm * slope, np.where(np.abs(mpre) <= dm, dm, 0.0)), f"{tag}m")
    m = r.m.astype(F64)
    pts = case.points.reshape(n, 3).astype(F64)
    for l, mt in enumerate(sn.mats):
        x = pts if l == 0 else r.h[l - 1].astype(F64)
        W, b = mt.W.astype(F64), mt.b.astype(F64)
        pre = x @ W.T + b
        dpre = dot_bound(x.shape[1] + 1, x.T, W.T) + (x.shape[1] + 3) * U * np.abs(b)
        rows_f, rows_p = slice(l * H, (l + 1) * H), slice((L + l) * H, (L + l + 1) * H)
        fraw = m @ Wm2[rows_f].T + bm2[rows_f]
        dfraw = dot_bound(257, m.T, Wm2[rows_f].T) + 259 * U * np.abs(bm2[rows_f])
        f = 15.0 * fraw + 30.0
        df = 15.0 * dfraw + U * (np.abs(15.0 * fraw) + np.abs(f))
        ph = m @ Wm2[rows_p].T + bm2[rows_p]
        dph = dot_bound(257, m.T, Wm2[rows_p].T) + 259 * U * np.abs(bm2[rows_p])
        arg = f * pre + ph
        assert np.abs(arg).max() <= ARG_MAX, (l, np.abs(arg).max())
        darg = np.abs(f) * dpre + np.abs(pre) * df + df * dpre + dph + 2 * U * (np.abs(f * pre) + np.abs(arg))
        cs, dcs = np.cos(arg), darg + COS_POLY
        p15, dp15 = 15.0 * pre, 15.0 * dpre + U * np.abs(15.0 * pre)
        factor, sc = _keep_rows(case, mt.drop, n, H)
        within(r.h[l], *_dropped(np.sin(arg), darg + SIN_POLY, factor, sc), f"{tag}y[{l}]")
        within(r.c[3 * l], *_dropped(cs, dcs, factor, sc), f"{tag}act_c[{3 * l}] cos")
        within(r.c[3 * l + 1], *_dropped(cs * f, _prod_bound(cs, dcs, f, df), factor, sc), f"{tag}act_c[{3 * l + 1}] cos freq")
        within(r.c[3 * l + 2], *_dropped(cs * p15, _prod_bound(cs, dcs, p15, dp15), factor, sc), f"{tag}act_c[{3 * l + 2}] cos 15 pre")


def _product(terms, identity=None):
    """sum of operand @ W over (operand (n, k_i), W (k_i, H)) pairs (+ identity rows): value and dot-product bound."""
    want = sum(op @ W for op, W in terms)
    k = sum(op.shape[1] for op, _ in terms) + (identity is not None)
    bound = sum(dot_bound(k, op.T, W) for op, W in terms)
    if identity is not None:
        want, bound = want + identity, bound + (k + 2) * U * np.abs(identity)
    return want, bound


def _times_cos(inc, c):
    want = inc[0] * c
    return want, np.abs(c) * inc[1] + 2 * U * np.abs(want)


def check_chain_rows(sn, case, out, tag="", npi_bound=None):
    """act_go, act_g (and G) and the gradient volumes, each from the stage's own stored act_go / act_g / act_c.  Returns the volumes'
    (value, bound) per level for the caller's second-call check."""
    r = StageRows(sn, case, out)
    n, H, npi, L = r.n, sn.H, r.npi, len(sn.kinds)
    up, so = case.upstream.reshape(n, 4).astype(F64), case.saved.reshape(n, 4).astype(F64)
    want, bound = up.copy(), np.zeros((n, 4))
    if sn.sigmoid:
        want[:, :3] = up[:, :3] * (so[:, :3] * (1.0 - so[:, :3]))
        bound[:, :3] = 3 * U * np.abs(want[:, :3])
    within(r.go, want, bound, f"{tag}act_go")
    assert np.array_equal(r.go[:, 3], case.upstream.reshape(n, 4)[:, 3]), "channel 3 of act_go is upstream itself"
    inc = _product([(r.go.astype(F64), sn.head_W.astype(F64))])
    if sn.pfilm:
        for l in range(L - 1, -1, -1):
            within(r.g[l], *_times_cos(inc, r.c[3 * l + 1].astype(F64)), f"{tag}act_g[{l}] g_pre")
            within(r.G[:, l * H:(l + 1) * H], *_times_cos(inc, r.c[3 * l + 2].astype(F64)), f"{tag}G freq[{l}]")
            within(r.G[:, (L + l) * H:(L + l + 1) * H], *_times_cos(inc, r.c[3 * l].astype(F64)), f"{tag}G phase[{l}]")
            if l:
                inc = _product([(r.g[l].astype(F64), sn.mats[l].W.astype(F64))])
        return []
    s = len(sn.mats) - 1
    op0 = None
    while s >= 0:
        mt = sn.mats[s]
        if mt.role == "fc2":                       # slabs s - 1 (fc1) and s (fc2) of one block
            gb, ga = r.g[s].astype(F64), r.g[s - 1].astype(F64)
            within(r.g[s], *_times_cos(inc, r.c[s].astype(F64)), f"{tag}act_g[{s}] fc2")
            inc2 = _product([(gb, mt.W.astype(F64))])
            within(r.g[s - 1], *_times_cos(inc2, r.c[s - 1].astype(F64)), f"{tag}act_g[{s - 1}] fc1")
            inc = _product([(ga, sn.mats[s - 1].W.astype(F64))], identity=gb)
            s -= 2
            continue
        within(r.g[s], *_times_cos(inc, r.c[s].astype(F64)), f"{tag}act_g[{s}]")
        op = r.g[s]
        if mt.film is not None:                    # the operand of the next product: one fp32 product, reproduced bit for bit
            op = op * np.repeat(case.freq[:, mt.film * H:(mt.film + 1) * H].astype(np.float32), npi, axis=0)
            assert op.dtype == np.float32
        op = op.astype(F64)
        if s:
            inc = _product([(op, mt.W.astype(F64))])
        else:
            op0 = op
        s -= 1
    assert op0 is not None, "layer 0 is a FiLM or sine layer"
    if sn.input == "position":
        return []
    # the gradient volumes: g_feat per input tile, scattered with the float64 weights of the float32 positions
    W0 = sn.mats[0].W.astype(F64)
    expect = []
    for lvl, vol in enumerate(case.levels):
        V, C = vol.shape[1], vol.shape[-1]
        want_v, bound_v = np.zeros((r.B, V, V, V, C)), np.zeros((r.B, V, V, V, C))
        for tk, (tl, cc) in enumerate(input_tiles(sn, case.levels)):
            if tl != lvl:
                continue
            Wc = W0[:, 32 * tk:32 * tk + 32]
            gfeat, dg = op0 @ Wc, dot_bound(H, op0.T, Wc)
            w_, b_ = scatter64(gfeat.reshape(r.B, npi, 32), dg, case.points, V, npi_bound or npi)
            want_v[..., cc:cc + 32], bound_v[..., cc:cc + 32] = w_, b_
        assert np.abs(want_v).max() > 0
        within(r.grad_vols[lvl], want_v, bound_v, f"{tag}grad volume level {lvl}")
        expect.append((want_v, bound_v))
    return expect


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
Z_DIM = 64
PYRAMID = [(7, 32), (4, 64), (3, 32)]        # (side, channels) per level
ONE_LEVEL = [(5, 32)]


def make_net(variant, H, seed):
    """(module on the CPU, (side, channels) of its volume levels) with random parameters from cnerf_amd.generators."""
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators import siren
    torch.manual_seed(seed)
    cls = getattr(siren, variant)
    spec = cls.spec
    levels = [] if spec.input == "position" else PYRAMID if spec.input == "pyramid" else ONE_LEVEL
    C = sum(c for _, c in levels)
    if spec.input in ("xyz", "position"):
        net = cls(3, 32 if spec.input == "xyz" else Z_DIM, H)
    else:
        net = cls(input_dim=C + (3 if spec.input == "feat_xyz" else 0), z_dim=C if spec.input_is_zdim else Z_DIM, hidden_dim=H)
    return net.eval(), levels


def random_case(net, levels, B, npi, seed, drop_p=0.0):
    """StageCase over all B images (saved is left to the caller: it is the forward's output) and the global feature's freq / phase."""
    g = torch.Generator().manual_seed(seed)
    vols = [(torch.randn((B, V, V, V, C), generator=g) * 0.5).numpy() for V, C in levels]
    freq = phase = None
    if net.spec.has_global:
        with torch.no_grad():
            freq, phase = (t.numpy() for t in net.film(torch.randn((B, Z_DIM), generator=g)))
    points = (torch.randn((B, npi, 3), generator=g) * 0.35).numpy()       # some beyond the 1.2 cube's faces: clamped corners
    upstream = torch.randn((B, npi, 4), generator=g).numpy()
    drop = None
    if drop_p:
        n_drop = sum(k != "res" for k in net.spec.layers)
        drop = (drop_p, (torch.rand((n_drop, B, npi, int(net.hidden_dim)), generator=g) >= drop_p).to(torch.uint8).numpy())
    return StageCase(vols, freq, phase, points, upstream, None, drop)


def chunk_of(case, image0, n_images):
    """The images [image0, image0 + n_images) of a case."""
    sl = slice(image0, image0 + n_images)
    cut = lambda t: None if t is None else np.ascontiguousarray(t[sl])
    drop = None if case.drop is None else (case.drop[0], np.ascontiguousarray(case.drop[1][:, sl]))
    return StageCase([cut(v) for v in case.levels], cut(case.freq), cut(case.phase), cut(case.points), cut(case.upstream), cut(case.saved), drop)
