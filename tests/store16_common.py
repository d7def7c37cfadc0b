"""The fp16 activation rows of the storing forward (field_h3_kernel<NT, STORE_TB16, HAS_RES, WF>, csrc/field_h3.hip: FiLM, plain-sine and
residual networks) row by row against float64: what tests/test_gpu_store16.py holds the kernels to and tests/test_store16_cpu.py shows an
honest float32 emulation to attain -- the sin slabs (X of every weight reduction), the cos slabs (the chain's derivative), the layer-0
input tiles.  Two launches store them: the render that keeps its activations (WF = 1 | 2, per-image folded weights) and the re-run of the
backward, cnerf_field_store16 = the launch chunk16 runs (WF = 0).  The scalar rules and layouts are those of tests/chain16_common.py
(f16, HF = h = 2^-11, FL = 2^-25, to_cos16, from_tb16) and tests/field_backward_stage_common.py (U = u = 2^-24, dot_bound, within).

(a) Equalities
--------------
layout      every stored element sits at the TB16 / COS16 index of csrc/bwd16.hpp (from_tb16, from_cos16 below); a buffer starts as a
            canary (0x7E5A: an fp16 NaN), so an element the launch did not store is not finite and one it stored elsewhere breaks a guard.
inputs      a feature tile equals fp16(clamp(x, +-65504)) of the fp32 lookup (ops.gather_features of the tile's 32 channels), bit for bit:
            shown for EVERY tile of every level, not level 0 alone -- the levels share the kernel's lookup code.  An xyz tile equals
            fp16 of the positions the pass reports in columns 0..2, zeros in 3..31.
rows past   the padded lanes of an image's last tile hold the rows of the image's LAST point, bit for bit, in feat, sin and cos
an image's  (tile_of_group() clamps the point index; the stores are gated by the wave's tile, not by the lane).  The issue that asked for
end         these tests expected them to keep the caller's bytes.  They must not: cnerf_weight_grad16 multiplies every row of a tile,
            padding included, by the chain's gradient rows, which are zero there -- 0 x (whatever an unwritten buffer held, NaN included)
            would reach dW.  So the contract is "finite, the last point's", and that is what is demanded.  A wave without a tile
            (tiles go in groups of four) has no block in the buffers and stores nothing: guards and the slots of other images keep
            their canary.
rgb_sigma   kept path: pixels, depth, coarse_ / fine_rgb_sigma of a render that keeps act16 equal those of the same render without;
            stage entry: rgb_sigma equals cnerf_field_forward in fp16x3 at the same positions (the non-storing WF = 0 instantiation).

(b) The pair identity
---------------------
s16 = fp16(s), c16 = fp16(c), s = sin A + e_s, c = cos A + e_c with |e| <= VSIN for ONE fp32 argument A:
    |s16^2 + c16^2 - 1| <= 2 h + 2 VSIN + h^2 + 4 FL
(two relative roundings: (1 + h)^2 - 1; 2 (|e_s sin| + |e_c cos|); the subnormal floor 2 FL (|s| + |c|)).  VSIN = 3.8e-7 is v_sin_f32's
recorded maximum behind the Cody-Waite reduction on |x| <= 300 (scripts/ubench/vsin_accuracy.hip, quoted in csrc/cnerf_dev.hpp); v_cos_f32
has no recorded figure of its own: it is the same unit a quarter revolution on, and the same figure is taken for it.  2 h dominates by
three orders of magnitude; no honest pair gets beyond 0.71 of it (two fp16 roundings cannot both be relatively worst at s^2 + c^2 = 1).

(c) Layer-local rows
--------------------
Slab m from what the launch itself stored for slab m - 1 (x^: the input tiles for m = 0), in float64 with the raw fp32 parameters:
    A = freq (W x^ + b) + phase,      a residual block's second matrix:  A = x^_in + W2 y^ + b2  (x^_in: the slab in front of fc1)
    |s16 - sin A| <= h |sin A| + FL + |cos A| d + d^2 / 2          |c16 - cos A| <= h |cos A| + FL + |sin A| d + d^2 / 2
    d = |freq| (sum_k |W_k| (h' |x^_k| + FL) + dot_bound(K)(|W|, |x^|) + 2^-19 sum_k |W_k x^_k|) [+ h' |x^_in| + FL]
        + 4 u (|freq W x^| + |freq b + phase| [+ |x^_in|] + pi) + VSIN
h' = h (1 + h): the stored operand is the fp16 rounding of the fp32 activation v the kernel multiplied, |v - x^| <= h |v| + FL.
2^-19: the operand is v as two TRUNCATED fp16 parts (h3_dev.hpp split_pair: the remainder of an 11-bit truncation, < 2^-10 |v|, again
truncated: 2^-20), the weights are two rounded parts (2^-22, once more for the per-image fold of the kept path), the dropped product of
the two low parts is < 2^-10 2^-11: 2^-20 + 2^-21 + 2^-21 = 2^-19 -- the issue's sketch had 2^-21, without the operand's truncation.
dot_bound(K): the matrix pipe's fp32 sum in any order, K the padded width.  4 u (...): the argument is never formed at full magnitude in
one piece -- the product part (times M = freq / 2 pi S rounded to fp32, reduced by an exact fma) and the constant part K = (freq b +
phase) / 2 pi (or bias and identity of a block) are rounded SEPARATELY before they meet, so each enters with its own magnitude (they may
cancel in A: 4 u |A| alone would not hold), pi for the reduced remainder.  The bound does not grow with depth.
Terms corrected on the hardware: none (see tests/test_gpu_store16.py for the measured ratios).

(d) End to end against the reference
------------------------------------
The stored sin rows of every slab against fp16 of the float64 network evaluated from the inputs (network() below in float64: the
oracle's field_mlp restated with its hidden activations kept).  Statistic per slab: share of elements more than one fp16 ulp (of the
float64 value) away, and the largest deviation in ulps.  Yardstick: the same statistic of the reference's OWN fp32 evaluation (network()
in float32: F.linear, freq * x + phase, sin -- three roundings at full magnitude) rounded to fp16.  Kernel share <= 2 x yardstick + 1e-3.
A case is usable only while the yardstick's share stays below 5 % at the last slab (tests/test_store16_cpu.py checks every case).
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import chain16_common as K
import field_backward_stage_common as S
from chain16_common import F16_MAX, FL, HF, f16, f32, from_tb16, idle_waves, to_cos16      # noqa: F401
from field_backward_stage_common import F64, U, dot_bound, lookup64, within                # noqa: F401

VSIN = 3.8e-7
CANARY16 = 0x7E5A                     # an fp16 NaN
TWO_PI = 2.0 * np.pi
PYRAMID4 = [(8, 32), (4, 64), (3, 32)]      # four feature tiles in three levels
ONE_LEVEL = [(8, 32)]
FAMILIES = ("SHORTSIREN_FG", "SHORTSIREN_F", "SHORTSIREN_FRes", "TALLSIREN_dRes", "TALLSIREN_dgx", "SHORTSIREN_FG_Pyrmd", "SHORTSIREN", "SingleSIREN_dg",
            "TALLSIREN_FG")
WIDE = ("SHORTSIREN_FG", "SHORTSIREN_FRes", "TALLSIREN_dgx")
NETS = [(v, 64) for v in FAMILIES] + [(v, H) for H in (128, 256) for v in WIDE]
B_RENDER, R_RENDER, S_RENDER = 3, 5, 14        # 350 points per image: 10 full tiles, a 30-row tile, one idle wave


def from_cos16(buf, nslab, tiles, NT):
    """COS16 (nslab, tiles, NT, 4 g, 64 = 32 h + j, 4 e) -> rows (nslab, tiles * 32, 32 NT): the inverse of to_cos16."""
    return np.ascontiguousarray(np.asarray(buf).reshape(nslab, tiles, NT, 4, 2, 32, 4).transpose(0, 1, 5, 2, 3, 4, 6)).reshape(nslab, tiles * 32, 32 * NT)


def to_tb16(rows, CT):
    """rows (nslab, tiles * 32, 32 CT) -> TB16 (nslab, tiles, CT, 32, 32) flat."""
    ns, n, _ = rows.shape
    return np.ascontiguousarray(rows.reshape(ns, n // 32, 32, CT, 32).transpose(0, 1, 3, 2, 4)).reshape(-1)


# ---- a network with its inputs, and one launch on it ----------------------------------------------------------------------------------------
@dataclass
class Case:
    variant: str
    sn: S.StageNet
    levels: List[tuple]                 # (side, channels)
    vols: List[np.ndarray]              # FULL (B, V, V, V, C) float32, channel-last
    freq: Optional[np.ndarray]          # FULL (B, n_film H) float32
    phase: Optional[np.ndarray]
    B: int

    @property
    def tiles_in(self):
        return S.input_tiles(self.sn, self.vols)

    @property
    def nslab(self):
        return len(self.sn.mats)

    def W0_padded(self, dtype):
        W0 = self.sn.mats[0].W.astype(dtype)
        out = np.zeros((W0.shape[0], 32 * len(self.tiles_in)), dtype)
        out[:, :W0.shape[1]] = W0
        return out


@dataclass
class Launch:
    """Images [image0, image0 + n_images) of the case; points (n_images, npi, 3) float32: the positions the pass reports."""
    image0: int
    n_images: int
    points: np.ndarray

    @property
    def npi(self):
        return self.points.shape[1]

    @property
    def tpi(self):
        return (self.npi + 31) // 32

    @property
    def tiles(self):
        return self.n_images * self.tpi

    @property
    def src(self):
        """(rows,) index into the chunk's (n_images * npi) points of every padded row: a padded lane reads its image's last point."""
        nn = np.minimum(np.arange(self.tpi * 32), self.npi - 1)
        return (np.arange(self.n_images)[:, None] * self.npi + nn[None]).reshape(-1)

    @property
    def valid(self):
        return np.tile(np.arange(self.tpi * 32) < self.npi, self.n_images)


def make_case(variant, H, seed=None, hot_feature=None):
    """Deterministic inputs (torch's CPU generator, NumPy's PCG64): images with distinct volumes, latents and FiLM vectors."""
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators import siren
    seed = sum(map(ord, variant)) + H if seed is None else seed
    spec = getattr(siren, variant).spec
    levels = [] if spec.input == "position" else PYRAMID4 if spec.input == "pyramid" else ONE_LEVEL
    net = K.make_net(variant, H, seed, levels)
    rng = np.random.default_rng(seed)
    B = B_RENDER
    vols = [(0.5 * rng.standard_normal((B, V, V, V, C))).astype(f32) for V, C in levels]
    if hot_feature is not None:
        vols[0][..., 5] = f32(hot_feature)
    freq = phase = None
    if spec.has_global:
        with torch.no_grad():
            freq, phase = (t.numpy().astype(f32) for t in net.film(torch.from_numpy(rng.standard_normal((B, K.Z_DIM)).astype(f32))))
    return Case(variant, S.stage_net(net), levels, vols, freq, phase, B), net


def random_points(cs, npi, seed):
    """Positions of a CPU-only launch (the GPU tests take the render's): some beyond the cube's faces."""
    return (np.random.default_rng(seed).standard_normal((cs.B, npi, 3)) * 0.35).astype(f32)


def film_rows(cs, la, m, dtype, wrong_image=False):
    """(freq, phase) rows (n_images * npi, H) of slab m; ones / zeros for a sine slab or a residual half."""
    H, film, n = cs.sn.H, cs.sn.mats[m].film, la.n_images * la.npi
    if film is None:
        return np.ones((n, H), dtype), np.zeros((n, H), dtype)
    img = np.repeat(np.arange(la.n_images), la.npi) + la.image0
    if wrong_image:
        img = np.where(img == la.image0 + 1, la.image0, img)
    return cs.freq[img, film * H:(film + 1) * H].astype(dtype), cs.phase[img, film * H:(film + 1) * H].astype(dtype)


def inputs64(cs, la):
    """Layer 0's input rows (n_images * npi, 32 n_in) by the float64 lookup at the fp32 positions."""
    n = la.n_images * la.npi
    x0 = np.zeros((n, 32 * len(cs.tiles_in)))
    for tk, (lvl, cc) in enumerate(cs.tiles_in):
        if lvl < 0:
            x0[:, 32 * tk:32 * tk + 3] = la.points.reshape(n, 3)
        else:
            x0[:, 32 * tk:32 * tk + 32] = lookup64(cs.vols[lvl][la.image0:la.image0 + la.n_images], la.points, cc)[0]
    return x0


def network(cs, la, x0, dtype):
    """The field network's hidden sines per slab [(n, H)] and rgb_sigma (n, 4) from the input rows x0, every operation in `dtype` in the
    reference's order: F.linear, freq * x + phase, sin; a residual block sin(x + fc2(sin(fc1 x)))."""
    sn = cs.sn
    hs, x = [], x0.astype(dtype)
    for m, mt in enumerate(sn.mats):
        W = cs.W0_padded(dtype) if m == 0 else mt.W.astype(dtype)
        pre = x @ W.T + mt.b.astype(dtype)
        if mt.role == "fc2":
            arg = hs[m - 2] + pre
        elif mt.film is not None:
            fr, ph = film_rows(cs, la, m, dtype)
            arg = fr * pre + ph
        else:
            arg = pre
        x = np.sin(arg)
        assert x.dtype == dtype
        hs.append(x)
    out = x @ sn.head_W.astype(dtype).T + sn.head_b.astype(dtype)
    if sn.sigmoid:
        out[:, :3] = dtype(1.0) / (dtype(1.0) + np.exp(-out[:, :3]))
    return hs, out


def ulp16(ref):
    """Spacing of fp16 at |ref| (subnormals: 2^-24)."""
    e = np.frexp(np.maximum(np.abs(np.asarray(ref, F64)), 2.0 ** -14))[1] - 1
    return np.ldexp(1.0, np.maximum(e, -14) - 10)


def ulp_stat(got, ref16):
    """(share of elements more than one fp16 ulp from ref16, the largest deviation in ulps)."""
    dev = np.abs(np.asarray(got, F64) - np.asarray(ref16, F64)) / ulp16(ref16)
    return float((dev > 1.0).mean()), float(dev.max())


def reference(cs, la):
    """(fp16 of the float64 network per slab [(n, H)], the yardstick [(share, max ulps)] of the reference's fp32 evaluation)."""
    x0 = inputs64(cs, la)
    ref = [f16(h) for h in network(cs, la, x0, F64)[0]]
    own = [f16(h) for h in network(cs, la, x0.astype(f32), f32)[0]]
    return ref, [ulp_stat(o, r) for o, r in zip(own, ref)]


# ---- float32 emulation of the storing launch --------------------------------------------------------------------------------------------------
HAZARDS = ("cos_quad_halves_swapped", "first_pair_from_previous_quad", "sincos_neighbour_channels", "slab_stride_of_the_call", "padded_lane_unclamped",
           "idle_wave_stores", "freq_wrong_image", "fc2_cos_without_identity", "leading_part_only", "input_unclamped")


def _trunc11(v):
    return (np.asarray(v, f32).view(np.uint32) & np.uint32(0xFFFFE000)).view(f32)


def _two_parts(v, truncate):
    """v as the sum of its two fp16 parts: truncated (activations, h3_dev.hpp) or rounded (packed weights)."""
    v = np.asarray(v, f32)
    hi = _trunc11(v) if truncate else f16(v)
    lo = v - hi
    return hi + (_trunc11(lo) if truncate else f16(lo))


def _r32(x):
    return np.asarray(x, F64).astype(f32)


def emulate(cs, la, hazard=None, storing=True):
    """One storing launch in float32 with fp16 at the stores.  Returns raw uint16 buffers feat / h / c (each with a canary tail of the
    call's size behind the chunk's: where a wrong slab stride or an idle wave lands), rgb_sigma (n, 4) float32 and the fp32 lookups per
    feature tile `gather` [(n, 32)] the input equality reads.  storing = False: the same arithmetic without buffers (the non-storing
    instantiation the stage's rgb_sigma must equal)."""
    assert hazard is None or hazard in HAZARDS
    sn, H, NT, nslab = cs.sn, cs.sn.H, cs.sn.H // 32, cs.nslab
    n_in, tpi, T = len(cs.tiles_in), la.tpi, la.tiles
    rows = T * 32
    pts_all = la.points.reshape(-1, 3)
    src = la.src.copy()
    if hazard == "padded_lane_unclamped":        # the lane reads point index >= npi: the next image's points (wrapping in the chunk)
        nn = np.arange(tpi * 32)
        src = ((np.arange(la.n_images)[:, None] * la.npi + nn[None]) % (la.n_images * la.npi)).reshape(-1)
    pts = pts_all[src]
    img_local = np.repeat(np.arange(la.n_images), tpi * 32)
    sub = Launch(la.image0, la.n_images, la.points)
    x064 = inputs64(cs, sub)
    x0_pts = _r32(x064)                                                 # the fp32 lookup of every real point
    x0 = x0_pts[src]
    if hazard == "padded_lane_unclamped":                               # ... looked up in the lane's own image's volume
        lane = Launch(la.image0, la.n_images, pts.reshape(la.n_images, tpi * 32, 3))
        x0 = _r32(inputs64(cs, lane))
    gather = [x0_pts[:, 32 * tk:32 * tk + 32] for tk, (lvl, _) in enumerate(cs.tiles_in) if lvl >= 0]
    clamped = np.clip(x0, f32(-F16_MAX), f32(F16_MAX))
    feat16 = x0.astype(np.float16) if hazard == "input_unclamped" else clamped.astype(np.float16)
    hs32, s16, c16 = [], [], []
    x = clamped
    for m, mt in enumerate(sn.mats):
        W = cs.W0_padded(f32) if m == 0 else mt.W
        S_w = f32(K.pow2_weight_scale(np.abs(W).max()))
        xs, Ws = _two_parts(x, True), _two_parts(W * S_w, False)
        if hazard == "leading_part_only" and m == min(1, nslab - 1):
            xs, Ws = f16(x), f16(W * S_w)
        acc = xs @ Ws.T                                                 # S (W x): fp32 sums of exact fp16 products
        film = mt.film
        fr = np.ones((rows, H), F64)
        ph = np.zeros((rows, H), F64)
        if film is not None:
            img = img_local + la.image0
            if hazard == "freq_wrong_image":
                img = np.where(img == la.image0 + 1, la.image0, img)
            fr, ph = cs.freq[img, film * H:(film + 1) * H].astype(F64), cs.phase[img, film * H:(film + 1) * H].astype(F64)
        if mt.role == "fc2":                                            # unfolded: fma(acc, 1 / S, b2), + x_in, Cody-Waite, revolutions
            a = _r32(acc.astype(F64) / float(S_w) + mt.b.astype(F64))
            a_id = _r32(_two_parts(hs32[m - 2], True).astype(F64) + a)
            u = _r32(a_id.astype(F64) / TWO_PI - np.rint(a_id.astype(F64) / TWO_PI))
            u_cos = u
            if hazard == "fc2_cos_without_identity":
                u_cos = _r32(a.astype(F64) / TWO_PI - np.rint(a.astype(F64) / TWO_PI))
        else:                                                           # folded: n = rint(acc Mh); u = fma(acc, Mh, -n) + K
            Mh = _r32(fr / (TWO_PI * float(S_w)))
            Kc = _r32((fr * mt.b.astype(F64) + ph) / TWO_PI)
            prod = acc.astype(F64) * Mh.astype(F64)
            u = _r32(_r32(prod - np.rint(_r32(prod).astype(F64))).astype(F64) + Kc)
            u_cos = u
        v, cv = _r32(np.sin(TWO_PI * u.astype(F64))), _r32(np.cos(TWO_PI * u_cos.astype(F64)))
        hs32.append(v)
        s16.append(v.astype(np.float16))
        c16.append(cv.astype(np.float16))
        x = v
    Wh = _two_parts(sn.head_W * f32(K.pow2_weight_scale(np.abs(sn.head_W).max())), False)
    out = _r32((_two_parts(x, True) @ Wh.T).astype(F64) / K.pow2_weight_scale(np.abs(sn.head_W).max()) + sn.head_b.astype(F64))
    if sn.sigmoid:
        out[:, :3] = f32(1.0) / (f32(1.0) + np.exp(-out[:, :3]))
    rgb_sigma = out[la.valid]
    if not storing:
        return dict(rgb_sigma=rgb_sigma)
    s16, c16 = np.stack(s16), np.stack(c16)
    quad = lambda a: a.reshape(nslab, rows, H // 8, 2, 4)               # channel 8 q + 4 h + e: (q, h, e); the lane half h owns a quad
    if hazard == "cos_quad_halves_swapped":
        c16 = quad(c16)[..., [2, 3, 0, 1]].reshape(nslab, rows, H)
    if hazard == "sincos_neighbour_channels":
        c16 = quad(c16)[..., [1, 0, 3, 2]].reshape(nslab, rows, H)
    if hazard == "first_pair_from_previous_quad":                       # ks / kc never refreshed: the quad's first pair is the previous quad's
        for a in (s16, c16):
            q = quad(a)
            q[:, :, 1:, :, :2] = q[:, :, :-1, :, :2].copy()
    # the buffers: the chunk's tiles, then a tail as large as the call's
    T_call = cs.B * tpi
    slab, slab_call = T * NT * 1024, T_call * NT * 1024
    bufs = dict(feat=np.full(T * n_in * 1024 + T_call * n_in * 1024, CANARY16, np.uint16),
                h=np.full(nslab * slab + nslab * slab_call, CANARY16, np.uint16), c=np.full(nslab * slab + nslab * slab_call, CANARY16, np.uint16))
    stride = slab_call if hazard == "slab_stride_of_the_call" else slab
    bufs["feat"][:T * n_in * 1024] = to_tb16(feat16[None], n_in).view(np.uint16)
    for m in range(nslab):
        bufs["h"][m * stride:m * stride + slab] = to_tb16(s16[m:m + 1], NT).view(np.uint16)
        bufs["c"][m * stride:m * stride + slab] = to_cos16(c16[m:m + 1], NT).view(np.uint16)
    if hazard == "idle_wave_stores":             # the wave without a tile stores the image's last point one tile past the image's end
        assert idle_waves(la.n_images, tpi) > 0
        for b in range(la.n_images):
            t_src, t_dst = (b + 1) * tpi - 1, (b + 1) * tpi
            last = slice(t_src * 32 + (la.npi - 1) % 32, t_src * 32 + (la.npi - 1) % 32 + 1)
            bufs["feat"][t_dst * n_in * 1024:(t_dst + 1) * n_in * 1024] = to_tb16(np.repeat(feat16[None, last], 32, axis=1), n_in).view(np.uint16)
            for m in range(nslab):
                o = m * slab + t_dst * NT * 1024
                bufs["h"][o:o + NT * 1024] = to_tb16(np.repeat(s16[m:m + 1, last], 32, axis=1), NT).view(np.uint16)
                bufs["c"][o:o + NT * 1024] = to_cos16(np.repeat(c16[m:m + 1, last], 32, axis=1), NT).view(np.uint16)
    return dict(bufs, rgb_sigma=rgb_sigma, gather=gather)


def decode(cs, la, bufs):
    """Raw fp16 buffers (uint16 or float16, the chunk's tiles first) -> dict(feat (rows, 32 n_in), h, c (nslab, rows, H)) float32, and
    `tail_intact`: whatever lies behind the chunk's tiles in the arrays still is the canary."""
    NT, nslab, n_in, T = cs.sn.H // 32, cs.nslab, len(cs.tiles_in), la.tiles
    out, intact = {}, True
    for k, n in (("feat", T * n_in * 1024), ("h", nslab * T * NT * 1024), ("c", nslab * T * NT * 1024)):
        raw = np.asarray(bufs[k]).view(np.uint16).reshape(-1)
        intact &= bool((raw[n:] == CANARY16).all())
        half = raw[:n].view(np.float16)
        out[k] = (from_tb16(half, 1, T, n_in)[0] if k == "feat" else from_tb16(half, nslab, T, NT) if k == "h" else from_cos16(half, nslab, T, NT)).astype(f32)
    out["tail_intact"] = intact
    return out


# ---- the check ----------------------------------------------------------------------------------------------------------------------------
def check(cs, la, out, ref=None, tag="", strict=True, inputs_only=False):
    """out: decode()'s rows (+ `gather`: the fp32 lookups [(n, 32)] per feature tile, `tail_intact`).  ref: reference(cs, la), shared.
    Returns {"pair[m]", "sin[m]", "cos[m]": worst |err| / bound, "e2e": [(share, max ulps, yardstick share, yardstick max)], "broken"}."""
    sn, H, nslab = cs.sn, cs.sn.H, cs.nslab
    valid, src = la.valid, la.src
    feat, h, c = (np.asarray(out[k], f32) for k in ("feat", "h", "c"))
    ratios, broken = {}, []

    def claim(cond, what):
        if strict:
            assert cond, tag + what
        elif not cond:
            broken.append(what)

    def held(got, want, bound, what):
        if strict:
            within(got, want, bound, tag + what)
        err = np.abs(np.asarray(got, F64) - want)
        ratios[what] = float(np.max(err / bound)) if np.isfinite(err).all() else np.inf

    claim(out.get("tail_intact", True), "memory behind the chunk's tiles was written")
    stored = not any(np.isnan(t[..., valid, :]).any() for t in (feat, h, c))
    claim(stored, "a row of the chunk was left unwritten (the canary is a NaN)")
    if not stored:                               # nothing below can be judged on NaN rows
        feat, h, c = (np.nan_to_num(t, nan=0.0, posinf=np.inf, neginf=-np.inf) for t in (feat, h, c))
    # rows past an image's end: the image's last point
    first = valid.nonzero()[0]                   # row of every real point of the chunk, in point order
    for k, t in (("feat", feat), ("h", h), ("c", c)):
        claim(np.array_equal(t[..., ~valid, :], t[..., first[src[~valid]], :], equal_nan=True), f"padded rows of {k} are not the image's last point")
    # input tiles
    pts = la.points.reshape(-1, 3)[src]
    g = iter(out["gather"])
    for tk, (lvl, cc) in enumerate(cs.tiles_in):
        got = feat[:, 32 * tk:32 * tk + 32]
        if lvl < 0:
            want = np.zeros((len(src), 32), f32)
            want[:, :3] = f16(pts)
        else:
            want = f16(np.clip(np.asarray(next(g), f32), f32(-F16_MAX), f32(F16_MAX)))[src]
        claim(np.array_equal(got, want), f"input tile {tk} (level {lvl}, channel {cc}) is not fp16(clamp(x))")
    if inputs_only:
        return dict(ratios, broken=broken)
    n_chunk = la.n_images * la.npi
    hv, cv, xv = h[:, valid].astype(F64), c[:, valid].astype(F64), feat[valid].astype(F64)
    h1 = HF * (1.0 + HF)
    for m, mt in enumerate(sn.mats):
        # (b) the pair identity
        pair = np.abs(hv[m] ** 2 + cv[m] ** 2 - 1.0)
        ratios[f"pair[{m}]"] = float(pair.max() / (2 * HF + 2 * VSIN + HF * HF + 4 * FL))
        claim(ratios[f"pair[{m}]"] <= 1.0, f"sin^2 + cos^2 of slab {m} is {ratios[f'pair[{m}]']:.3g} x its bound from 1")
        # (c) from the launch's own previous slab
        xh = xv if m == 0 else hv[m - 1]
        W = (cs.W0_padded(F64) if m == 0 else mt.W.astype(F64))
        fr, ph = film_rows(cs, la, m, F64)
        assert len(fr) == n_chunk
        Wx = xh @ W.T
        prod, const = fr * Wx, fr * mt.b.astype(F64) + ph
        aW = np.abs(W)
        d = np.abs(fr) * ((h1 * np.abs(xh) + FL) @ aW.T + dot_bound(W.shape[1], np.abs(xh).T, aW.T) + 2.0 ** -19 * (np.abs(xh) @ aW.T))
        if mt.role == "fc2":
            xin = hv[m - 2]
            const = const + xin
            d = d + h1 * np.abs(xin) + FL
        A = prod + const
        d = d + 4 * U * (np.abs(prod) + np.abs(fr * mt.b.astype(F64) + ph) + (np.abs(hv[m - 2]) if mt.role == "fc2" else 0.0) + np.pi) + VSIN
        sA, cA = np.sin(A), np.cos(A)
        held(hv[m], sA, HF * np.abs(sA) + FL + np.abs(cA) * d + d * d / 2, f"sin[{m}]")
        held(cv[m], cA, HF * np.abs(cA) + FL + np.abs(sA) * d + d * d / 2, f"cos[{m}]")
    # (d) end to end
    ref16, yard = ref if ref is not None else reference(cs, la)
    e2e = []
    for m in range(nslab):
        share, worst = ulp_stat(hv[m], ref16[m])
        e2e.append((share, worst, yard[m][0], yard[m][1]))
        claim(share <= 2 * yard[m][0] + 1e-3, f"slab {m}: {share:.4f} of the sines are beyond one fp16 ulp of float64, the reference's own fp32 has {yard[m][0]:.4f}")
    claim(yard[-1][0] < 0.05, "the case is unusable: the reference's own fp32 share at the last slab is 5 % or more")
    return dict(ratios, e2e=e2e, broken=broken)


def far_from_other_image(cs, la, out, ref16):
    """Median |stored sine of the chunk's first image - float64 sine of its SECOND image| over the median |sine| of the latter, at slab 0
    (the sines of a plain hidden layer are small whatever the image): images are distinguishable."""
    hv = np.asarray(out["h"], F64)[0, la.valid]
    other = ref16[0][la.npi:2 * la.npi].astype(F64)
    return float(np.median(np.abs(hv[:la.npi] - other)) / np.median(np.abs(other)))
