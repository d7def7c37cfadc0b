"""The fp16 rows of the per-point FiLM storing forward (csrc/field_pw16.hip: field_pw16_kernel<NT, STORE = true>, then pw_deriv_kernel<NT>)
row by row against float64: what tests/test_gpu_store_pw16.py holds the kernels to and tests/test_store_pw16_cpu.py shows an honest
float32 emulation to attain.  Two launches store the rows: the render that keeps its activations (aux->act16 with amax) and the re-run
of the backward, cnerf_field_store_pw16 = the launch chunk_pw16 runs.  Scalar rules, layouts and helpers are those of
tests/store16_common.py (f16, HF = h = 2^-11, FL = 2^-25, U = u = 2^-24, VSIN, dot_bound, from_tb16, from_cos16, lookup64, the canary);
the float64 network is field_backward_stage_common._check_forward_pfilm's, restated with the bounds of THIS arithmetic.

Notation: x = the looked-up feature in fp32 clamped to +-65504 (known bit for bit: (a)), p = the fp32 position, m~ = LeakyReLU_0.2(Wm1 x
+ bm1), fr~_l = Wm2[l H ..] m~ + bm2, ph~_l = Wm2[(L + l) H ..] m~ + bm2, f = 15 fr + 30, pre_l = W_l y_{l-1} + b_l (y_{-1} = p),
A_l = f_l pre_l + ph_l; y16 / c16 / m16: the stored fp16 rows; h' = h (1 + h).

(a) Equalities
--------------
layout      every element at its TB16 / COS16 index; every buffer between guards, starting as the fp16 NaN canary (amax, rgb_sigma: fp32
            NaN): every element of every tile of the chunk is finite afterwards, nothing behind the chunk's tiles is written.  A wave
            without a tile has no block in any buffer (the tiles of an image are dense: image b's tiles end where image b + 1's begin),
            so "the blocks an idle wave would have stay untouched" is: the first tile of the next image holds that image's own rows
            (conditions (c), (e) there) and the guards and the canary behind the chunk's last tile are intact -- there is no separate
            check by wave.
inputs      feature tile = fp16(clamp(x, +-65504)) of the fp32 lookup bit for bit; position tile = fp16 (nearest even) of the pass's
            positions in columns 0..2, zeros in 3..31.
padded      the padded lanes of an image's last tile hold the image's LAST point's rows bit for bit in feat, y, m, all 3 L slabs of c and
            amax (tile_of_group() clamps the point index; pw_deriv_kernel reads what the forward stored for the lane).
rgb_sigma   stage: equals cnerf_field_forward in fp16x3; kept: the render's outputs do not change when it keeps act16.
repeat      two launches on the same inputs give the same bits in every buffer.

(b) Pair identity     |y16^2 + c16^2 - 1| <= 2 h + 2 VSIN + h^2 + 4 FL, store16's bound: ONE reduced argument feeds v_sin_f32 and v_cos_f32.

(c) m, y_l, cos_l: layer-local
------------------------------
A product of the matrix pipe, acc = S (W v) from the fp32 operand v: v as two TRUNCATED fp16 parts (2^-20 |v|, and 2^-24 absolute where
the low part falls under fp16's smallest number), S W as two ROUNDED parts (2^-22, and 2^-25 / S absolute), the product of the two low
parts dropped (2^-21), the fp32 sum in any order over the padded width K:
    E(v, W; K) = 2^-19 |W| |v| + 2^-24 sum_k |W_k| + (2^-25 / S) sum_k |v_k| + dot_bound(K + 1)(|W|, |v|) + (K + 3) u |b|
(the accumulator starts from S b rounded once and carries it through the K additions).
m           d_m~ = E(x, Wm1; 32), times the slope, + u |m~| (the 0.2 product); the stored m16 is within h |m~| + FL + d_m of m~, with
            either slope where |Wm1 x + bm1| <= d_m~.  m~, fr~, ph~ are taken from the fp32 FEATURE, never from m16: the kernel multiplies
            the fp32 m in two parts, and a bound carrying h sum |Wm2| |m16| would not see the low part go missing.
fr, ph      d_fr = |Wm2| d_m + E(m, Wm2 rows; 256) with |m| <= |m~| + d_m;  d_f = 15 (d_fr + u (|fr~ + 2| + d_fr)): the 2 S_f is added
            to the FINISHED accumulator, one rounding at the magnitude of fr + 2.
pre_0       from the fp32 position, exact: d_pre = E(p, W_0; 32).
pre_l       l >= 1, from the launch's own y16_{l-1}: the kernel multiplied the fp32 value v that y16 rounds, |v - y16| <= h' |y16| + FL:
            d_pre = |W| (h' |y16| + FL) + E((1 + h') |y16| + FL, W_l; H).
argument    d = |f| d_pre + |pre| d_f + d_f d_pre + d_ph + u (2 |f pre| + 2 |ph| + |A|) + VSIN: q = (accf + 2 S_f) accp is one
            product (u |f pre|), c1 and c2 are fp32 constants (u |f pre|, u |ph|), ph c2 is rounded (u |ph|), the fma once at the magnitude
            of the argument (u |A|); the reduction u - rint(u) is exact.
rows        |y16 - sin A| <= h |sin A| + FL + |cos A| d + d^2 / 2, and the twin for cos.  |A| <= 300 is asserted (VSIN's range).

(e) Derivative rows and amax, from exactly what pw_deriv_kernel read
---------------------------------------------------------------------
f^ = 15 (Wm2[fr rows] m16 + bm2) + 30, p^ = 15 (W_l y16_{l-1} + b_l) (layer 0: fp16 of the position) in float64; want c16 f^ and c16 p^
clamped to +-65504.  The kernel multiplies the LEADING fp16 part of each scaled weight, which pack_h3_kernel ROUNDS to nearest
((_Float16)(S W): relative h, 2^-25 / S absolute), by the exact fp16 operand:
    d_f^ = 15 (h |W| |m16| + (2^-25 / S) sum |m16| + dot_bound(257) + 259 u |bm2| + u |fr^ + 2|) + u |f^|     (the product with kf = 15 / S_f)
    d_p^ likewise with K = H (32 for layer 0), without the 2 S_f
    |stored - c16 f^| <= |c16| d_f^ + u |c16 f^| + h |c16 f^| + FL        (the fp32 product with cos, one fp16 store)
amax        D = the largest stored |cos f|, |cos 15 pre| of the point's 2 H: max(1, D) / (1 + h) - FL <= amax <= max(1, D) / (1 - h) + FL;
            amax == 1.0 exactly wherever D (1 + h) + FL < 1; D <= amax (1 + h) everywhere (the chain's contract); finite and below 3e38.

(d) End to end, default-initialised networks only: store16's statistic and rule on the stored y_l (share beyond one fp16 ulp of fp16 of
the float64 network <= 2 x the same share of the reference's own fp32 evaluation + 1e-3; usable while that yardstick stays below 5 % at
the last layer).  The range net is excluded: its fp32 evaluation is chaotic by layer 3.

Terms corrected on the hardware: none (see tests/test_gpu_store_pw16.py for the measured ratios).
"""
from dataclasses import dataclass

import numpy as np

import chain_pw16_common as P
import field_backward_stage_common as S
import store16_common as K16
from store16_common import (B_RENDER, CANARY16, F16_MAX, F64, FL, HF, U, VSIN, Launch, dot_bound, f16, f32, from_cos16, from_tb16, lookup64, to_cos16,
                            to_tb16, ulp_stat)
from store16_common import R_RENDER, S_RENDER, random_points      # noqa: F401  (re-exported to the two test files)

TWO_PI = 2.0 * np.pi
SLOPE = float(f32(0.2))
V_SIDE = 8
HOT_VOXEL = 4                        # (4, 4, 4) of image 1: its centre is the point (0.075, 0.075, 0.075)
HOT_CENTRE = 0.6 * ((2 * HOT_VOXEL + 1) / V_SIDE - 1.0)
PAIR_BOUND = 2 * HF + 2 * VSIN + HF * HF + 4 * FL
#       name        kind       H    layers
NETS = {
    "default64":  ("default", 64, 8), "default128": ("default", 128, 8), "default256": ("default", 256, 8),
    "short2":     ("default", 64, 2), "short1": ("default", 64, 1),
    "range64":    ("range", 64, 8), "range256": ("range", 256, 8),
    "quiet":      ("quiet", 64, 8),
    "hot":        ("hot", 64, 8),
}
E2E = ("default64", "default128", "default256", "short2", "short1", "hot")      # default-initialised: (d) applies


@dataclass
class Case:
    name: str
    kind: str
    sn: S.StageNet
    vol: np.ndarray                     # FULL (B, V, V, V, 32) float32, channel-last
    B: int

    @property
    def L(self):
        return len(self.sn.mats)

    @property
    def e2e(self):
        return self.name in E2E


def make_case(name):
    """Deterministic inputs: (Case, the module)."""
    import torch
    kind, H, L = NETS[name]
    seed = sum(map(ord, name))
    net = P.make_net(H, L, seed)
    with torch.no_grad():
        w2, b2 = net.mapping_network.network[2].weight, net.mapping_network.network[2].bias
        if kind == "range":
            for l in range(1, L):
                net.network[l].layer.weight *= 8.0
            w2 *= 4.0
        if kind == "quiet":
            w2[:L * H] *= 2.0 ** -10
            b2[:L * H] = -2.0
            # (weights AND biases of the layers: the biases are torch's default, up to 1 / sqrt(fan in) -- 15 b_0 alone reaches 8.7)
            for l in range(L):
                net.network[l].layer.weight *= 1.0 / (8 if l else 32)
                net.network[l].layer.bias *= 1.0 / (8 if l else 32)
    rng = np.random.default_rng(seed)
    vol = (0.5 * rng.standard_normal((B_RENDER, V_SIDE, V_SIDE, V_SIDE, 32))).astype(f32)
    if kind == "hot":
        vol[1, HOT_VOXEL, HOT_VOXEL, HOT_VOXEL] = (1e5 * (-1.0) ** np.arange(32)).astype(f32)
    return Case(name, kind, S.stage_net(net), vol, B_RENDER), net


def hot_points(points):
    """points (n, 3) -> those within reach of the hot voxel (one of their eight corners, with the lookup's own uncertainty)."""
    ic = np.clip(((points.astype(F64) / S.HALF_VOXEL + 1.0) * V_SIDE - 1.0) / 2.0, 0.0, V_SIDE - 1.0)
    return (np.abs(ic - HOT_VOXEL) < 1.0 + 1e-3).all(axis=1)


def hot_rows(cs, la):
    """(n_images * npi,) bool: the chunk's points that read the hot voxel (image 1 of the call)."""
    out = np.zeros((la.n_images, la.npi), bool)
    if cs.kind == "hot" and la.image0 <= 1 < la.image0 + la.n_images:
        out[1 - la.image0] = hot_points(la.points[1 - la.image0])
    return out.reshape(-1)


def lookup(cs, la):
    """float64 lookup (n_images * npi, 32) at the launch's fp32 positions."""
    return lookup64(cs.vol[la.image0:la.image0 + la.n_images], la.points, 0)[0]


def map_rows(cs, l):
    sn, H, L = cs.sn, cs.sn.H, cs.L
    Wm2, bm2 = sn.map[2], sn.map[3]
    return Wm2[l * H:(l + 1) * H], bm2[l * H:(l + 1) * H], Wm2[(L + l) * H:(L + l + 1) * H], bm2[(L + l) * H:(L + l + 1) * H]


def network(cs, la, x0, dtype):
    """The reference's evaluation in `dtype`, its order (siren.py): m, per layer F.linear, 15 fr + 30, f * pre + ph, sin.  -> [y_l], max |A|, max |cos f|, |cos 15 pre|."""
    sn = cs.sn
    Wm1, bm1 = sn.map[0].astype(dtype), sn.map[1].astype(dtype)
    mp = x0.astype(dtype) @ Wm1.T + bm1
    m = np.where(mp > 0, mp, mp * dtype(0.2))
    x = la.points.reshape(-1, 3).astype(dtype)
    ys, amax, dmax = [], 0.0, 0.0
    cool = ~hot_rows(cs, la)
    for l, mt in enumerate(sn.mats):
        Wf, bf, Wp, bp = (t.astype(dtype) for t in map_rows(cs, l))
        f = (m @ Wf.T + bf) * dtype(15.0) + dtype(30.0)
        ph = m @ Wp.T + bp
        pre = x @ mt.W.astype(dtype).T + mt.b.astype(dtype)
        arg = f * pre + ph
        amax = max(amax, float(np.abs(arg[cool]).max()))
        dmax = max(dmax, float(np.abs(np.cos(arg[cool]) * f[cool]).max()), float(np.abs(np.cos(arg[cool]) * dtype(15.0) * pre[cool]).max()))
        x = np.sin(arg)
        assert x.dtype == dtype
        ys.append(x)
    return ys, amax, dmax


def reference(cs, la):
    """(fp16 of the float64 network per layer, the yardstick [(share, max ulps)] of the reference's own fp32 evaluation, max |A|, the largest |cos f|, |cos 15 pre|); the
    yardstick and the maxima over the points out of the hot voxel's reach."""
    x0 = lookup(cs, la)
    r64, amax, dmax = network(cs, la, x0, F64)
    ref = [f16(y) for y in r64]
    own = [f16(y) for y in network(cs, la, x0.astype(f32), f32)[0]]
    cool = ~hot_rows(cs, la)
    return ref, [ulp_stat(o[cool], r[cool]) for o, r in zip(own, ref)], amax, dmax


# ---- float32 emulation of the two kernels --------------------------------------------------------------------------------------------------
HAZARDS = ("cos_own_reduction", "f_without_30", "operand_low_part_dropped", "deriv_rows_of_previous_tile", "phase_rows_at_next_layer", "deriv_pre_from_y_l",
           "deriv_low_pieces", "stale_unit_second_trip", "amax_one_lane_half", "amax_without_floor", "m_before_leaky", "padded_rows_unwritten",
           "position_tile_tail", "position_truncated", "cos_slab_stride_1")


def _trunc11(v):
    return (np.asarray(v, f32).view(np.uint32) & np.uint32(0xFFFFE000)).view(f32)


def _r32(x):
    return np.asarray(x, F64).astype(f32)


def _scale(W):
    return f32(K16.K.pow2_weight_scale(np.abs(W).max()))


def _mm3(v, W, b, drop_low=False):
    """S (W v + b) as the matrix pipe forms it: (S, fp32 accumulator) -- operand in two truncated parts, S W in two rounded parts, three
    products, started from fp32(S b)."""
    Sw = _scale(W)
    v = np.asarray(v, f32)
    vh = _trunc11(v)
    vl = _trunc11(v - vh)
    Ws = (W * Sw).astype(f32)
    Wh = f16(Ws)
    Wl = f16(Ws - Wh)
    acc = _r32(b.astype(F64) * float(Sw)) + vh @ Wh.T + vh @ Wl.T
    if not drop_low:
        acc = acc + vl @ Wh.T
    return Sw, acc.astype(f32)


def _hi(v, W, b):
    """pw_deriv_kernel: the leading (rounded) part of S W times the exact fp16 operand, from fp32(S b)."""
    Sw = _scale(W)
    return Sw, (_r32(b.astype(F64) * float(Sw)) + np.asarray(v, f32) @ f16((W * Sw).astype(f32)).T).astype(f32)


def _lo(v, W, b):
    Sw = _scale(W)
    Ws = (W * Sw).astype(f32)
    return Sw, (_r32(b.astype(F64) * float(Sw)) + np.asarray(v, f32) @ f16(Ws - f16(Ws)).T).astype(f32)


def emulate(cs, la, hazard=None):
    """One storing launch in float32 with fp16 at the stores.  Returns raw buffers: feat / h / c uint16 (each with a canary tail of the
    call's size behind the chunk's), amax float32 (L, tiles * 32) with NaN where nothing was stored, rgb_sigma (n, 4), `gather` (n, 32)
    the fp32 lookup, and `f_rel` / `p_rel`: the largest relative error, per element with |value| >= 1, of pw_deriv's f and 15 pre before the cosine and the store."""
    assert hazard is None or hazard in HAZARDS
    sn, H, L = cs.sn, cs.sn.H, cs.L
    NT, tpi, T = H // 32, la.tpi, la.tiles
    rows = T * 32
    src, valid = la.src, la.valid
    Wm1, bm1 = sn.map[0], sn.map[1]
    gather = _r32(lookup(cs, la))
    x = np.clip(gather, f32(-F16_MAX), f32(F16_MAX))[src]
    pts = la.points.reshape(-1, 3)[src]
    feat16 = np.zeros((rows, 64), np.float16)
    feat16[:, :32] = x.astype(np.float16)
    feat16[:, 32:35] = (_trunc11(pts) if hazard == "position_truncated" else pts).astype(np.float16)
    if hazard == "position_tile_tail":
        feat16[:, 35:] = feat16[:, 3:32]
    # the mapping hidden layer
    S1, acc = _mm3(x, Wm1, bm1)
    v = acc / S1
    m32 = np.clip(np.where(v > 0, v, v * f32(0.2)), f32(-F16_MAX), f32(F16_MAX)).astype(f32)
    m16 = (v if hazard == "m_before_leaky" else m32).astype(np.float16)
    p32 = np.zeros((rows, 32), f32)
    p32[:, :3] = np.clip(pts, f32(-F16_MAX), f32(F16_MAX))
    group = (np.arange(rows) // 32 % tpi) // 4 + (np.arange(rows) // 32 // tpi) * ((tpi + 3) // 4)
    second_trip = group >= (group.max() + 2) // 2          # a grid of half as many blocks as groups: each block's second group
    ys32, y16, c16 = [], [], []
    xin = p32
    for l, mt in enumerate(sn.mats):
        Wf, bf, Wp, bp = map_rows(cs, l)
        if hazard == "phase_rows_at_next_layer":
            Wp, bp = sn.map[2][(l + 1) * H:(l + 2) * H], sn.map[3][(l + 1) * H:(l + 2) * H]
        low = hazard == "operand_low_part_dropped"
        Sf, accf = _mm3(m32, Wf, bf, low)
        Sph, accph = _mm3(m32, Wp, bp, low)
        if hazard == "stale_unit_second_trip" and l == 0:  # fr of output tile 1 reads the slot ph of tile 0 still occupies
            accf[second_trip, 32:64] = _mm3(m32, Wp, bf)[1][second_trip, :32]
        W = np.zeros((H, 32), f32) if l == 0 else mt.W
        if l == 0:
            W[:, :3] = mt.W
        Sp, accp = _mm3(xin, W, mt.b)
        q = ((accf + f32(2.0) * Sf).astype(f32) * accp).astype(f32)
        c1, c2 = _r32(15.0 / (TWO_PI * float(Sf) * float(Sp))), _r32(1.0 / (TWO_PI * float(Sph)))
        t2 = (accph * c2).astype(f32)
        u = _r32(q.astype(F64) * float(c1) + t2.astype(F64))
        a = (u - np.rint(u)).astype(f32)
        a_cos = a
        if hazard == "cos_own_reduction":                  # the product part reduced alone: the phase term never reaches the cosine
            pc = _r32(q.astype(F64) * float(c1))
            a_cos = (pc - np.rint(pc)).astype(f32)
        s, c = _r32(np.sin(TWO_PI * a.astype(F64))), _r32(np.cos(TWO_PI * a_cos.astype(F64)))
        ys32.append(s)
        y16.append(s.astype(np.float16))
        c16.append(c.astype(np.float16))
        xin = s
    Sh, acch = _mm3(xin, sn.head_W, np.zeros(4, f32))
    out = _r32(acch.astype(F64) / float(Sh) + sn.head_b.astype(F64))
    if sn.sigmoid:
        out[:, :3] = f32(1.0) / (f32(1.0) + np.exp(-out[:, :3]))
    first = valid.nonzero()[0]
    rgb_sigma = out[first]
    # pw_deriv_kernel on the stored rows
    c_slabs = np.full((3 * L, rows, H), np.nan, np.float16)
    for l in range(L):
        c_slabs[l if hazard == "cos_slab_stride_1" else 3 * l] = c16[l]
    amax = np.ones((L, rows), f32)
    f_rel = p_rel = 0.0
    mm = _lo if hazard == "deriv_low_pieces" else _hi
    pos16 = np.zeros((rows, 32), f32)
    pos16[:, :3] = f16(pts)                                # (formed again from the fp32 position, not read from the stored tile)
    with np.errstate(invalid="ignore"):
        for l, mt in enumerate(sn.mats):
            Wf, bf, _, _ = map_rows(cs, l)
            Sf, accf = mm(m16.astype(f32), Wf, bf)
            k2 = f32(0.0) if hazard == "f_without_30" else f32(2.0) * Sf
            fv = ((accf + k2).astype(f32) * (f32(15.0) / Sf)).astype(f32)
            W = np.zeros((H, 32), f32) if l == 0 else mt.W
            if l == 0:
                W[:, :3] = mt.W
            xop = pos16 if l == 0 else y16[l if hazard == "deriv_pre_from_y_l" else l - 1].astype(f32)
            Sp, accp = mm(xop, W, mt.b)
            pv = (accp * (f32(15.0) / Sp)).astype(f32)
            if hazard is None:
                f64_, p64_ = 15.0 * (m16.astype(F64) @ Wf.astype(F64).T + bf) + 30.0, 15.0 * (xop.astype(F64) @ W.astype(F64).T + mt.b)
                for got, ref64, which in ((fv, f64_, 0), (pv, p64_, 1)):      # per element, where |value| >= 1 (the GPU line's rule)
                    big = np.abs(ref64) >= 1.0
                    rel = float(np.max(np.abs(got - ref64)[big] / np.abs(ref64)[big])) if big.any() else 0.0
                    f_rel, p_rel = (max(f_rel, rel), p_rel) if which == 0 else (f_rel, max(p_rel, rel))
            cl = c_slabs[3 * l].astype(f32)
            cf = np.clip((cl * fv).astype(f32), f32(-F16_MAX), f32(F16_MAX))
            cp = np.clip((cl * pv).astype(f32), f32(-F16_MAX), f32(F16_MAX))
            both = np.maximum(np.abs(cf), np.abs(cp))
            if hazard == "amax_one_lane_half":
                both = both[:, (np.arange(H) % 8) < 4]
            am = np.fmax.reduce(both, axis=1)
            amax[l] = am if hazard == "amax_without_floor" else np.fmax(f32(1.0), am)
            if hazard == "deriv_rows_of_previous_tile":
                cf, cp = np.roll(cf, 32, axis=1), np.roll(cp, 32, axis=1)
            c_slabs[3 * l + 1], c_slabs[3 * l + 2] = cf.astype(np.float16), cp.astype(np.float16)
    y16 = np.stack(y16)
    if hazard == "padded_rows_unwritten":
        nan16 = np.array([CANARY16], np.uint16).view(np.float16)[0]
        feat16[~valid], m16[~valid], y16[:, ~valid], c_slabs[:, ~valid] = nan16, nan16, nan16, nan16
        amax[:, ~valid] = np.nan
    T_call = cs.B * tpi
    tail = lambda n: np.full(n, CANARY16, np.uint16)
    bufs = dict(feat=np.concatenate([to_tb16(feat16[None], 2).view(np.uint16), tail(T_call * 2048)]),
                h=np.concatenate([to_tb16(y16, NT).view(np.uint16), to_tb16(m16[None], 8).view(np.uint16), tail(T_call * (L * NT + 8) * 1024)]),
                c=np.concatenate([to_cos16(c_slabs, NT).view(np.uint16), tail(T_call * 3 * L * NT * 1024)]))
    return dict(bufs, amax=amax, rgb_sigma=rgb_sigma, gather=gather, f_rel=f_rel, p_rel=p_rel)


def decode(cs, la, bufs):
    """Raw buffers (the chunk's tiles first) -> dict(feat (rows, 64), y (L, rows, H), m (rows, 256), c (3 L, rows, H), amax (L, rows))
    float32, and `tail_intact`."""
    NT, L, T = cs.sn.H // 32, cs.L, la.tiles
    out, intact = {}, True
    raw = {k: np.ascontiguousarray(np.asarray(bufs[k])).view(np.uint16).reshape(-1) for k in ("feat", "h", "c")}
    n_y = L * T * NT * 1024
    for k, n in (("feat", T * 2048), ("h", n_y + T * 8 * 1024), ("c", 3 * n_y)):
        intact &= bool((raw[k][n:] == CANARY16).all())
    out["feat"] = from_tb16(raw["feat"][:T * 2048].view(np.float16), 1, T, 2)[0].astype(f32)
    out["y"] = from_tb16(raw["h"][:n_y].view(np.float16), L, T, NT).astype(f32)
    out["m"] = from_tb16(raw["h"][n_y:n_y + T * 8 * 1024].view(np.float16), 1, T, 8)[0].astype(f32)
    out["c"] = from_cos16(raw["c"][:3 * n_y].view(np.float16), 3 * L, T, NT).astype(f32)
    am = np.asarray(bufs["amax"], f32).reshape(-1)
    intact &= bool(np.isnan(am[L * T * 32:]).all())
    out["amax"] = am[:L * T * 32].reshape(L, T * 32)
    out["tail_intact"] = intact
    return out


# ---- the check ----------------------------------------------------------------------------------------------------------------------------
def _E(v_abs, W, b, K):
    """E(v, W; K) of the docstring: (rows, n_out)."""
    aW = np.abs(W.astype(F64))
    Sw = float(_scale(W))
    return (2.0 ** -19 * (v_abs @ aW.T) + 2.0 ** -24 * aW.sum(axis=1)[None] + (2.0 ** -25 / Sw) * v_abs.sum(axis=1)[:, None] + dot_bound(K + 1, v_abs.T, aW.T)
            + (K + 3) * U * np.abs(b.astype(F64))[None])


def _hi_bound(v_abs, W, b, K):
    aW = np.abs(W.astype(F64))
    return HF * (v_abs @ aW.T) + (2.0 ** -25 / float(_scale(W))) * v_abs.sum(axis=1)[:, None] + dot_bound(K + 1, v_abs.T, aW.T) + (K + 3) * U * np.abs(b.astype(F64))[None]


def check(cs, la, out, ref=None, tag="", strict=True):
    """out: decode()'s rows plus `gather` (n, 32): the fp32 lookup of the chunk's points.  ref: reference(cs, la), shared; None skips (d).
    Returns {"pair", "m", "sin", "cos", "cosf", "cosp", "amax": worst |err| / bound, "f_rel", "p_rel": the stored derivative rows'
    largest relative error (fp16 store included), "e2e": [(share, max ulps, yardstick share, yardstick max)], "Amax", "broken"}."""
    sn, H, L = cs.sn, cs.sn.H, cs.L
    valid, src = la.valid, la.src
    feat, y, m, c, amax = (np.asarray(out[k], f32) for k in ("feat", "y", "m", "c", "amax"))
    ratios, broken = {}, []

    def claim(cond, what):
        if strict:
            assert cond, tag + what
        elif not cond:
            broken.append(what)

    def held(got, want, bound, what, keep=None):
        err = np.abs(np.asarray(got, F64) - want)
        ok = np.isfinite(err)
        r = np.where(ok, err / np.maximum(bound, 1e-300), np.inf)
        r = np.where(ok & (err == 0), 0.0, r)
        if keep is not None:
            r = r[keep]
        worst = float(r.max()) if r.size else 0.0
        ratios[what.split("[")[0]] = max(ratios.get(what.split("[")[0], 0.0), worst)
        claim(worst <= 1.0, f"{what} is {worst:.3g} x its bound from float64")

    claim(out.get("tail_intact", True), "memory behind the chunk's tiles was written")
    stored = all(np.isfinite(t).all() for t in (feat, y, m, c, amax))
    claim(stored, "an element of the chunk's tiles is not finite (the canary is a NaN)")
    claim(bool((amax[np.isfinite(amax)] < 3e38).all()), "amax is 3e38 or more")
    if not stored:
        feat, y, m, c, amax = (np.nan_to_num(t, nan=0.0, posinf=F16_MAX, neginf=-F16_MAX) for t in (feat, y, m, c, amax))
    # (a) rows past an image's end: the image's last point
    first = valid.nonzero()[0]
    for k, t in (("feat", feat), ("y", y), ("m", m), ("c", c)):
        claim(np.array_equal(t[..., ~valid, :], t[..., first[src[~valid]], :], equal_nan=True), f"padded rows of {k} are not the image's last point")
    claim(np.array_equal(amax[:, ~valid], amax[:, first[src[~valid]]], equal_nan=True), "padded rows of amax are not the image's last point")
    # (a) input tiles
    gather = np.asarray(out["gather"], f32)
    xc = np.clip(gather, f32(-F16_MAX), f32(F16_MAX))
    bits = lambda t: np.ascontiguousarray(t, f32).astype(np.float16).view(np.uint16)       # (array_equal alone takes -0.0 for +0.0)
    claim(np.array_equal(bits(feat[:, :32]), bits(f16(xc)[src])), "the feature tile is not fp16(clamp(x))")
    pts = la.points.reshape(-1, 3)
    want = np.zeros((len(src), 32), f32)
    want[:, :3] = f16(pts)[src]
    claim(np.array_equal(bits(feat[:, 32:35]), bits(want[:, :3])), "the position tile is not fp16 (nearest even) of the positions")
    claim(not bits(feat[:, 35:]).any(), "columns 3..31 of the position tile are not zero")
    # the chunk's real points from here on
    yv, cv, mv, av = y[:, valid].astype(F64), c[:, valid].astype(F64), m[valid].astype(F64), amax[:, valid].astype(F64)
    cool = ~hot_rows(cs, la)                     # every point out of the hot voxel's reach
    h1 = HF * (1.0 + HF)
    # (b)
    pair = np.abs(yv ** 2 + cv[0::3] ** 2 - 1.0)
    ratios["pair"] = float(pair.max() / PAIR_BOUND)
    claim(ratios["pair"] <= 1.0, f"sin^2 + cos^2 is {ratios['pair']:.3g} x its bound from 1")
    # (c) m from the fp32 feature
    x = xc.astype(F64)
    Wm1, bm1 = sn.map[0], sn.map[1]
    mpre = x @ Wm1.astype(F64).T + bm1
    slope = np.where(mpre > 0, 1.0, SLOPE)
    mt_ = mpre * slope
    dmp = _E(np.abs(x), Wm1, bm1, 32)
    dm = dmp * slope + U * np.abs(mt_)
    near0 = np.abs(mpre) <= dmp
    dm = np.where(near0, dmp + U * np.abs(mpre), dm)              # either slope: both values lie within d_m~ of zero's side
    held(mv, np.clip(mt_, -F16_MAX, F16_MAX), HF * np.abs(mt_) + FL + dm, "m", keep=cool)
    am_ = np.abs(mt_) + dm
    p = pts.astype(F64)
    Amax = 0.0
    pos16 = f16(pts).astype(F64)
    f_rel = p_rel = 0.0
    for l, mt in enumerate(sn.mats):
        Wf, bf, Wp, bp = map_rows(cs, l)
        fr = mt_ @ Wf.astype(F64).T + bf
        ph = mt_ @ Wp.astype(F64).T + bp
        dfr = dm @ np.abs(Wf.astype(F64)).T + _E(am_, Wf, bf, 256)
        dph = dm @ np.abs(Wp.astype(F64)).T + _E(am_, Wp, bp, 256)
        f = 15.0 * fr + 30.0
        df = 15.0 * (dfr + U * (np.abs(fr + 2.0) + dfr))
        W, b = mt.W.astype(F64), mt.b.astype(F64)
        if l == 0:
            pre = p @ W.T + b
            dpre = _E(np.abs(p), mt.W, mt.b, 32)
        else:
            xh = yv[l - 1]
            pre = xh @ W.T + b
            vb = h1 * np.abs(xh) + FL
            dpre = vb @ np.abs(W).T + _E(np.abs(xh) + vb, mt.W, mt.b, H)
        A = f * pre + ph
        Amax = max(Amax, float(np.abs(A[cool]).max()))
        d = np.abs(f) * dpre + np.abs(pre) * df + df * dpre + dph + U * (2 * np.abs(f * pre) + 2 * np.abs(ph) + np.abs(A)) + VSIN
        sA, cA = np.sin(A), np.cos(A)
        held(yv[l], sA, HF * np.abs(sA) + FL + np.abs(cA) * d + d * d / 2, f"sin[{l}]", keep=cool)
        held(cv[3 * l], cA, HF * np.abs(cA) + FL + np.abs(sA) * d + d * d / 2, f"cos[{l}]", keep=cool)
        # (e) from what pw_deriv_kernel read
        c16 = cv[3 * l]
        frh = mv @ Wf.astype(F64).T + bf
        fh = 15.0 * frh + 30.0
        dfh = 15.0 * (_hi_bound(np.abs(mv), Wf, bf, 256) + U * np.abs(frh + 2.0)) + U * np.abs(fh)
        xop = pos16 if l == 0 else yv[l - 1]
        ph_ = 15.0 * (xop @ W.T + b)
        Wk = mt.W if l else np.concatenate([mt.W, np.zeros((H, 29), f32)], axis=1)
        xk = xop if l else np.concatenate([xop, np.zeros((len(xop), 29))], axis=1)
        dphh = 15.0 * _hi_bound(np.abs(xk), Wk, mt.b, 32 if l == 0 else H) + U * np.abs(ph_)
        for k, val, dv, name in ((1, fh, dfh, "cosf"), (2, ph_, dphh, "cosp")):
            wv = c16 * val
            held(cv[3 * l + k], np.clip(wv, -F16_MAX, F16_MAX), np.abs(c16) * dv + (U + HF) * np.abs(wv) + FL, f"{name}[{l}]", keep=cool)
            big = cool[:, None] & (np.abs(wv) >= 1.0) & (np.abs(wv) < F16_MAX)
            if big.any():
                rel = float(np.max(np.abs(cv[3 * l + k] - wv)[big] / np.abs(wv)[big]))
                f_rel, p_rel = (max(f_rel, rel), p_rel) if k == 1 else (f_rel, max(p_rel, rel))
        # amax
        D = np.maximum(np.abs(cv[3 * l + 1]), np.abs(cv[3 * l + 2])).max(axis=1)
        D1 = np.maximum(1.0, D)
        lo_, hi_ = D1 / (1 + HF) - FL, D1 / (1 - HF) + FL
        a_l = av[l]
        r = np.maximum((lo_ - a_l) / (D1 * HF), (a_l - hi_) / (D1 * HF))      # excess in units of the rounding allowance: > 0 fails
        ratios["amax"] = max(ratios.get("amax", 0.0), float(np.max(np.abs(a_l - D1) / (D1 * HF / (1 - HF) + FL))))
        claim(bool((r <= 0).all()), f"amax[{l}] is outside max(1, D) / (1 +- h) -+ FL")
        must1 = D * (1 + HF) + FL < 1.0
        claim(bool((a_l[must1] == 1.0).all()), f"amax[{l}] is not exactly 1 where every stored derivative is below 1")
        claim(bool((D <= a_l * (1 + HF)).all()), f"amax[{l}]: a stored derivative exceeds amax (1 + h)")
    claim(Amax <= 300.0, f"|A| reaches {Amax:.1f}: beyond the range of VSIN")
    for k in ("sin", "cos", "cosf", "cosp", "m"):
        ratios.setdefault(k, 0.0)
    ratios.update(f_rel=f_rel, p_rel=p_rel, Amax=Amax)
    # hot points: finite and inside fp16's range (the finiteness claim above covers every row)
    claim(bool((np.abs(m) <= F16_MAX).all() and (np.abs(c) <= F16_MAX).all()), "m or a derivative row is beyond +-65504")
    # (d)
    e2e = []
    if ref is not None and cs.e2e:
        ref16, yard = ref[:2]
        for l in range(L):
            share, worst = ulp_stat(yv[l][cool], ref16[l][cool])
            e2e.append((share, worst, yard[l][0], yard[l][1]))
            claim(share <= 2 * yard[l][0] + 1e-3, f"layer {l}: {share:.4f} of the sines are beyond one fp16 ulp of float64, the reference's own fp32 has {yard[l][0]:.4f}")
        claim(yard[-1][0] < 0.05, "the case is unusable: the reference's own fp32 share at the last layer is 5 % or more")
    return dict(ratios, e2e=e2e, broken=broken)


def summary(r):
    """One line of a launch's figures."""
    line = "worst |err| / bound " + " ".join(f"{k} {r[k]:.3f}" for k in ("pair", "m", "sin", "cos", "cosf", "cosp", "amax"))
    line += f"; |A| <= {r['Amax']:.1f}; stored cos f / cos 15 pre relative error (fp16 store included) {r['f_rel']:.2e} / {r['p_rel']:.2e}"
    if r.get("e2e"):
        l, e = max(enumerate(r["e2e"]), key=lambda le: le[1][0])
        line += f"; (d) layer {l} share {e[0]:.4f} ({e[1]:.0f} ulps), reference's fp32 {e[2]:.4f} ({e[3]:.0f} ulps)"
    return line


def long_shape(cus):
    """(R, S) of the long case (B = 2 images, pass 2, R R S points per image): B ceil(tiles per image / 4) tile groups are about 2.5 x
    the CU count and no multiple of 8 (the eight group classes differ in length), the last tile is ragged; S <= 128 as check_cfg wants."""
    want = 5 * cus // 4                          # groups per image
    best = None
    for R in range(2, 65):
        for S_ in range(2, 129):
            npi = R * R * S_
            G = ((npi + 31) // 32 + 3) // 4
            if npi % 32 == 0 or (2 * G) % 8 == 0:
                continue
            key = (abs(G - want) // 4, 4 * G == (npi + 31) // 32, abs(G - want), R, S_)      # close to 2.5, and with an idle wave if one can be had
            if best is None or key < best[0]:
                best = (key, R, S_)
    return best[1], best[2]
