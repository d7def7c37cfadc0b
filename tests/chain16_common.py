"""The half-precision gradient chain (cnerf_field_chain16 -> chain16_kernel<NT, DRY, HAS_RES>, csrc/bwd16.hip) row by row in float64: the
expectation and its derived bound, a float32 NumPy emulation of the kernel's arithmetic (honest, or with one named hazard), the NumPy
restatement of which tile groups a dry run samples, and the cases shared by tests/test_chain16_cpu.py and tests/test_gpu_chain16.py.

Every check is LAYER-LOCAL, as in tests/field_backward_stage_common.py: the expected row of slab m comes from what the stage itself
stored one step earlier (go' of the inputs for the last slab, g16[m + 1] / S_{m+1} otherwise), so no error is amplified through the
network and every element is held to the rounding of ONE step.  h = 2^-11 (fp16 unit roundoff), u = 2^-24, FL = 2^-25 (half the spacing
of fp16's subnormals: the absolute floor of a conversion, in the units the converted number has).

What the kernel does per point (row), in the order of bwd16.hip
---------------------------------------------------------------
    go' = upstream * s (1 - s) (channels 0..2 with CNERF_F_SIGMOID_RGB), fp32; gs = go' S_go; go16 = fp16(gs); the head product's
          operand is fp16(gs) + fp16(gs - fp16(gs))
    slab m (last .. 0):  acc = W_{m+1}^T operand_{m+1} (+ the identity fragments of the block above, re-scaled), fp32 sums of exact
          fp16 x fp16 products;  ac = acc cos_m;  stored g16[m] = fp16(clamp(ac U S_m));  operand_m = fp16(ac freq_m U T_m)
          U = winv_{m+1} / T_{m+1} un-scales the accumulator, S_m is the slab's stored scale (a power of two for the whole call, from
          the dry run's sampled maximum), T_m = 2^14 / (bound on the point's |gp_m|) rounded down to a power of two: per POINT.
    layer 0: gin = (W_0^T operand_0) winv_0 / T_0 in fp32, true units (or its trilinear scatter into the gradient volumes).
All scales are powers of two: products with them are exact unless they leave fp32's range, which the magnitudes here never do.

Derivations
-----------
go16      three fp32 roundings (3 u relative; none for channel 3 and without the sigmoid), then one fp16 conversion of gs:
              bound(go16, stored units) = (3 u + h) |gs| + FL;   channels 4..31 and rows past an image's end: exactly 0.
head      the operand is go' to 3 u (its fp32 roundings) + 2^-22 (the low part's own fp16 rounding: h h |gs|) + FL / S_go;
product   head^T is packed as fp16(W s): h |W| + FL / s per weight (s: the matrix' power-of-two scale; the floor matters for weights
          2^-14 below the matrix' largest); 8 product terms in two MFMAs: dot_bound(8).
operand   of slab m + 1, against the STORED row ga^ = g16[m+1] / S_{m+1}: the stored value and the MFMA operand are two fp16
          conversions of the same fp32 number ac (times freq: one fp32 rounding each way), so
              |operand / T - ga^ freq| <= (2 h + 3 u) |gp| + |freq| FL / S_{m+1} + FL / T,     gp = ga^ freq.
          T is taken ONE BINADE BELOW the float64 value of pow2_to_2p14(bound) (bound from the stored rows' maximum, which is within h
          of the kernel's), so a knife-edge exponent cannot decide a failure.
product   d inc = d gp |W| + |gp| (h |W| + FL / s) + dot_bound(H)(|gp|, |W|); the fp32 accumulation of the matrix pipe is held to the
          bound of a length-H sum in any order.
identity  of a residual block (slab m + 2 = fc2 feeds the slab below fc1 directly): the fragments kept in registers are fc2's operand,
          i.e. ga^_fc2 to (2 h + 3 u) |ga_fc2| + FL / S_{m+2} + FL / T_{m+2}; their re-scaling is a power of two (exact) and the add is
          one fused multiply-add: + u |inc + identity|.
slab m    want = cos_m (inc + identity); the epilogue's product with the cosine is one fp32 rounding (3 u allowed), the store one fp16
          conversion at scale S_m:
              bound(g16[m], true units) = |cos| (d inc + d identity) + 3 u |want| + h |want| + FL / S_m.
          A clamped element (the sampled maximum missed its tile: the sampling case) is exactly +-65504 in stored units.
gin       the same product bound with W_0's columns of the input tile, no cosine, no fp16 store: d inc + 3 u |want|.
volume    own-atomics path: scatter64 of tests/field_backward_stage_common.py with d g = the gin bound -- its "volume" terms cover
          the fp32 trilinear weights, the products and any order of the atomics -- plus k u |base| for a non-zero base
          (tests/scatter_patch_common.py); a voxel no sample's neighbourhood holds keeps its base bit for bit.
copies    Every scale that follows a point is a power of two derived from the point's own maximum, so the chain of a point times 2^-k is
          the point's chain times 2^-k BIT FOR BIT from the first operand on, provided the head operand itself is exact: upstream values
          of 8 bits and no sigmoid (fp16's subnormals still hold them 2^-24 below the call's largest).  The cases "copies_*" demand
          that equality of the gin rows: it is what "tiny-gradient points keep 11 bits" and "the identity term is re-scaled exactly"
          mean.  It carries the per-tile-scale hazard, which a span of 2^24 leaves at 2.6 x the row bound: the stored rows' own floor
          FL / S, which every layer-local bound must contain, is as coarse there as that hazard's FL / T.
scales    S_m = pow2_scales_kernel's rule (the maximum lands in (2^10, 2^11]) applied to the float64 maximum of the SAMPLED rows' want,
          exactly -- asserted only after checking that this maximum sits further from a power of two than the row bound;  gmax[m] lies
          within the largest pre-store row bound of the sampled rows of that maximum.  "gmax is never below a stored value": the
          conversion is monotonic, so fp16(gmax[m] S_m) >= every stored |value| of a sampled row (gmax itself may lie below a value
          that was rounded UP on its way into fp16).  The head's scale comes from max |upstream| over the WHOLE chunk (an exact maximum).
Terms corrected on the hardware: none (see tests/test_gpu_chain16.py for the measured ratios).

Sampled groups (field_common.hpp group_range(), chain16_kernel).  Groups of 4 consecutive tiles of one image, G = ceil(tiles per image
/ 4) per image; class c of 8 owns the groups [total c / 8, total (c + 1) / 8); block i of a class starts at the class's first group +
i * step and strides by (blocks of the class) * step: whatever the number of blocks, the union is every step-th group from the class's
first.
"""
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import field_backward_stage_common as S
from field_backward_stage_common import F64, U, dot_bound, within      # noqa: F401  (within, dot_bound: re-exported to the tests)
from scatter_patch_common import addend_count

f32 = np.float32
HF = 2.0 ** -11
FL = 2.0 ** -25
F16_MAX = 65504.0
Z_DIM = 64


# ---- the kernels' scalar rules --------------------------------------------------------------------------------------------------------
def f16(x):
    """fp32 -> fp16 -> fp32, round to nearest even (v_cvt_f16_f32)."""
    return np.asarray(x, f32).astype(np.float16).astype(f32)


def pow2_weight_scale(wmax):
    """bwd16.hpp: 2^floor(log2(16384 / max|W|)) (max |W| s in [2^13, 2^14))."""
    wmax = f32(wmax)
    if not (wmax > 1e-30 and wmax < 3e38):
        return 1.0
    e = int(np.frexp(f32(16384.0) / wmax)[1])
    return float(2.0 ** min(e - 1, 100))


def pow2_to_2p14(bound):
    """bwd16.hpp: T = 2^(14 - e), bound = m 2^e with m in [0.5, 1); 0 / denormal / huge -> 1.  Any float dtype, elementwise."""
    bound = np.asarray(bound)
    e = np.frexp(bound)[1].astype(np.int64)
    ok = (bound >= 1e-30) & (14 - e > -127) & (14 - e < 128)
    return np.where(ok, np.ldexp(np.ones(bound.shape, bound.dtype), np.where(ok, 14 - e, 0)), 1.0).astype(bound.dtype)


def pow2_scale_rule(g):
    """grad_kernels.hip pow2_scales_kernel: S = 2^(11 - ceil(log2 g)); 1 where g is 0."""
    g = float(g)
    if not (g > 0.0 and g < 3e38):
        return 1.0
    m, e = np.frexp(g)
    return float(2.0 ** int(np.clip(11 - (e - 1 if m == 0.5 else e), -100, 100)))


def pow2_distance(g):
    """Relative distance of g > 0 to the nearest power of two."""
    m = np.frexp(float(g))[0]                  # [0.5, 1)
    return min(m - 0.5, 1.0 - m) / m


# ---- which tile groups a dry run samples ----------------------------------------------------------------------------------------------
def production_step(n_images, tpi):
    return int(np.clip(n_images * ((tpi + 3) // 4) // 2048, 1, 16))


def sampled_groups(n_images, tpi, step):
    total = n_images * ((tpi + 3) // 4)
    return [g for c in range(8) for g in range(total * c // 8, total * (c + 1) // 8, step)]


def tiles_of_groups(groups, tpi):
    """Tile indices (image * tpi + tile of the image) the four waves of a block work on for these groups: idle waves own none."""
    G = (tpi + 3) // 4
    return sorted((g // G) * tpi + (g % G) * 4 + w for g in groups for w in range(4) if (g % G) * 4 + w < tpi)


def idle_waves(n_images, tpi):
    return n_images * (4 * ((tpi + 3) // 4) - tpi)


# ---- buffer layouts (csrc/bwd16.hpp) --------------------------------------------------------------------------------------------------
def to_cos16(rows, NT):
    """rows (nslab, tiles * 32, H) -> COS16 (nslab, tiles, NT, 4, 64, 4) flat: channel 32 t + 8 g + 4 h + e of point j sits in lane j + 32 h."""
    ns, n, H = rows.shape
    return np.ascontiguousarray(rows.reshape(ns, n // 32, 32, NT, 4, 2, 4).transpose(0, 1, 3, 4, 5, 2, 6)).reshape(-1)


def from_tb16(buf, nslab, tiles, CT):
    """TB16 (nslab, tiles, CT, 32 points, 32 channels) -> rows (nslab, tiles * 32, 32 CT)."""
    return np.ascontiguousarray(np.asarray(buf).reshape(nslab, tiles, CT, 32, 32).transpose(0, 1, 3, 2, 4)).reshape(nslab, tiles * 32, 32 * CT)


# ---- a case -----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """One call on the chunk's images.  Arrays hold the chunk only unless they say FULL: rows = n_images * tpi * 32 padded rows (image b,
    point nn -> row b * tpi * 32 + nn)."""
    name: str
    sn: S.StageNet
    levels: List[tuple]                 # (side, channels) of the volume levels
    B: int
    R: int
    Sr: int
    pss: int
    image0: int
    n_images: int
    group_step: int
    upstream: np.ndarray                # FULL (B, npi, 4) float32
    saved: np.ndarray                   # FULL (B, npi, 4) float32
    freq: Optional[np.ndarray]          # FULL (B, n_film H) float32
    cos: np.ndarray                     # (nslab, rows, H) float16
    points: np.ndarray                  # FULL (B, npi, 3) float32 (read by pass 2; the ray passes form their own)
    hot: Optional[tuple] = None         # sampling case: (image of the chunk, point) of the one huge upstream row
    base: Optional[List[np.ndarray]] = None      # pass 2 with a volume: what the chunk's gradient volumes hold before the call
    copies: int = 0                     # > 0: point nn is point nn - nn % copies times 2^-(nn % copies), cosines included (exact inputs)

    @property
    def npi(self):
        return self.R * self.R * self.Sr

    @property
    def tpi(self):
        return (self.npi + 31) // 32

    @property
    def rows(self):
        return self.n_images * self.tpi * 32

    @property
    def valid(self):
        return np.tile(np.arange(self.tpi * 32) < self.npi, self.n_images)

    @property
    def nslab(self):
        return len(self.sn.mats)

    def pad(self, t, fill_last=False):
        """FULL (B, npi, k) -> the chunk's padded rows (rows, k); padding rows are 0, or (fill_last) the image's last point."""
        t = t[self.image0:self.image0 + self.n_images]
        out = np.zeros((self.n_images, self.tpi * 32, t.shape[-1]), t.dtype)
        out[:, :self.npi] = t
        if fill_last:
            out[:, self.npi:] = t[:, -1:]
        return out.reshape(self.rows, -1)

    def unpad(self, rows):
        return rows.reshape(self.n_images, self.tpi * 32, -1)[:, :self.npi].reshape(self.n_images * self.npi, -1)

    def freq_rows(self, m, dtype=F64, image_of=None):
        """(rows, H) FiLM frequencies of slab m (ones for a sine / residual slab)."""
        H, film = self.sn.H, self.sn.mats[m].film
        if film is None:
            return np.ones((self.rows, H), dtype)
        fr = self.freq[self.image0:self.image0 + self.n_images, film * H:(film + 1) * H].astype(dtype)
        img = np.repeat(np.arange(self.n_images), self.tpi * 32) if image_of is None else image_of
        return fr[img]

    def fmax_rows(self, dtype=F64):
        """(rows, nslab): max(1, max |freq|) of the row's image per FiLM slab, 1 elsewhere (lds_fmax)."""
        out = np.ones((self.rows, self.nslab), dtype)
        for m in range(self.nslab):
            if self.sn.mats[m].film is not None:
                out[:, m] = np.maximum(1.0, np.abs(self.freq_rows(m, dtype)).max(axis=1))
        return out

    def feature_tiles(self):
        """[(level, first channel)] of layer 0's feature input tiles (the xyz tile has no rows)."""
        return [(i, c) for i, (_, ch) in enumerate(self.levels) for c in range(0, ch, 32)]

    def W0_padded(self, dtype):
        W0 = self.sn.mats[0].W.astype(dtype)
        n_in = len(S.input_tiles(self.sn, [np.zeros((1, 1, 1, 1, c)) for _, c in self.levels]))
        out = np.zeros((W0.shape[0], 32 * n_in), dtype)
        out[:, :W0.shape[1]] = W0
        return out


def weight_scales(sn):
    """(winv per slab then the head's, ||W||_1 per slab then the head's) as the packing forms them, float32."""
    mats = [m.W for m in sn.mats] + [sn.head_W]
    winv = np.array([1.0 / pow2_weight_scale(np.abs(W).max()) for W in mats], f32)
    anorm = np.array([np.abs(W).astype(f32).sum(axis=0, dtype=f32).max() for W in mats], f32)
    return winv, anorm


def go_prime(cs, dtype):
    """d loss / d head pre-activation of the padded rows, (rows, 4): zero on padding rows."""
    up, so = cs.pad(cs.upstream).astype(dtype), cs.pad(cs.saved).astype(dtype)
    go = up.copy()
    if cs.sn.sigmoid:
        go[:, :3] = up[:, :3] * (so[:, :3] * (dtype(1.0) - so[:, :3]))
    return go


# ---- float32 emulation of the kernel ----------------------------------------------------------------------------------------------------
HAZARDS = ("cos_quad_half", "film_prev_slab", "film_image0", "identity_dropped", "identity_prev_T", "scale_per_tile", "stale_weight_unit",
           "padded_lane_stores", "gmax_slab_shift")


def _chain32(cs, S_slab, S_go, hazard):
    """One launch of the chain on all tiles in float32 with fp16 at the two conversion points.  Returns stored go16 (rows, 4), stored g
    (nslab, rows, H), per-row max |ga| in true units gm (nslab, rows), gomax (rows), gin (feature tiles, rows, 32), clamp count."""
    sn, nslab, H, rows = cs.sn, cs.nslab, cs.sn.H, cs.rows
    winv, anorm = weight_scales(sn)
    go = go_prime(cs, f32)
    if hazard == "padded_lane_stores":            # `if (!valid) go = 0` forgotten: the padded lane repeats the image's last point
        up, so = cs.pad(cs.upstream, True), cs.pad(cs.saved, True)
        go = up.copy()
        if sn.sigmoid:
            go[:, :3] = up[:, :3] * (so[:, :3] * (f32(1.0) - so[:, :3]))
    gs = np.clip(go * f32(S_go), f32(-60000.0), f32(60000.0))
    hi = f16(gs)
    lo = f16(gs - hi)
    gomax = np.abs(go).max(axis=1)
    W16 = [f16(m.W * f32(1.0 / winv[i])) for i, m in enumerate(sn.mats)]
    Wh16 = f16(sn.head_W * f32(1.0 / winv[nslab]))
    fmax = cs.fmax_rows(f32)
    img = np.repeat(np.arange(cs.n_images), cs.tpi * 32)
    if hazard == "film_image0":
        img = np.where(img == 1, 0, img)
    cosr = cs.cos.astype(f32)
    if hazard == "cos_quad_half":                 # the second dword of a cos quad folded onto the first
        cosr = cosr.reshape(nslab, rows, H // 4, 4)[..., [0, 1, 0, 1]].reshape(nslab, rows, H)
    n_film = sn.n_film

    def per_tile(bound):
        return np.repeat(bound.reshape(-1, 32).max(axis=1), 32) if hazard == "scale_per_tile" else bound

    stored, gm = np.zeros((nslab, rows, H), f32), np.zeros((nslab, rows), f32)
    sat = 0
    z = lo @ Wh16 + hi @ Wh16
    Uacc = np.full(rows, winv[nslab] / f32(S_go), f32)
    T = pow2_to_2p14(per_tile(fmax[:, nslab - 1] * anorm[nslab] * gomax))
    op = skip_frag = T_skip = skip_max = gpmax = None
    for m in range(nslab - 1, -1, -1):
        if m < nslab - 1:
            skip = m + 2 < nslab and sn.mats[m + 2].role == "fc2"
            Uacc = winv[m + 1] / T
            Wm = W16[m + 1]
            if hazard == "stale_weight_unit" and m == 0 and nslab >= 3:      # output tile 0 multiplied by the previous matrix' unit
                Wm = Wm.copy()
                Wm[:, :32] = W16[m + 2][:, :32]
            z = op @ Wm
            if skip and hazard != "identity_dropped":
                kskip = (f32(1.0) / winv[m + 1] * np.ones(rows, f32)) if hazard == "identity_prev_T" else T / (T_skip * winv[m + 1])
                z = z + skip_frag * kskip[:, None]
            Tn = pow2_to_2p14(per_tile(fmax[:, m] * (anorm[m + 1] * gpmax + (skip_max if skip else f32(0.0)))))
        else:
            Tn = T
        ac = z * cosr[m]
        US, UT = Uacc * f32(S_slab[m]), Uacc * Tn
        stored[m] = f16(np.clip(ac * US[:, None], f32(-F16_MAX), f32(F16_MAX)))
        film = sn.mats[m].film
        if film is not None and hazard == "film_prev_slab":
            film = (film - 1) % n_film
        fr = np.ones((rows, H), f32) if film is None else cs.freq[cs.image0:cs.image0 + cs.n_images, film * H:(film + 1) * H][img]
        op = f16((ac * fr) * UT[:, None])
        vm = np.abs(ac).max(axis=1) * US
        gm[m] = vm / f32(S_slab[m])
        gpmax = gm[m] * fmax[:, m]
        sat += int((vm.reshape(-1, 32) > F16_MAX).any(axis=1).sum())
        if sn.mats[m].role == "fc2":
            skip_frag, T_skip, skip_max = op, Tn, gpmax
        T = Tn
    W0 = f16(cs.W0_padded(f32) * f32(1.0 / winv[0]))
    U0 = winv[0] / T
    gin = np.stack([(op @ W0[:, 32 * tk:32 * tk + 32]) * U0[:, None] for tk in range(len(cs.feature_tiles()))]) if cs.feature_tiles() else None
    return hi, stored, gm, gomax, gin, sat


def emulate(cs, hazard=None):
    """The stage's outputs (the dict check() reads) from a float32 emulation: head scale, dry run over the sampled groups, scales, chain."""
    assert hazard is None or hazard in HAZARDS
    nslab = cs.nslab
    upmax = float(np.abs(cs.upstream[cs.image0:cs.image0 + cs.n_images]).max())
    S_go = pow2_scale_rule(upmax)
    _, _, gm, gomax, _, _ = _chain32(cs, np.ones(nslab), S_go, hazard)
    step = cs.group_step or production_step(cs.n_images, cs.tpi)
    tiles = tiles_of_groups(sampled_groups(cs.n_images, cs.tpi, step), cs.tpi)
    srow = (np.asarray(tiles)[:, None] * 32 + np.arange(32)).reshape(-1)
    gmax = np.zeros(nslab + 2, f32)
    gmax[:nslab] = gm[:, srow].max(axis=1)
    if hazard == "gmax_slab_shift":               # the maximum of slab m lands in slot m + 1
        gmax[1:nslab + 1] = gmax[:nslab].copy()
        gmax[0] = 0.0
    gmax[nslab], gmax[nslab + 1] = gomax[srow].max(), upmax
    S_slab = np.array([pow2_scale_rule(g) for g in gmax[:nslab]])
    hi, stored, _, _, gin, sat = _chain32(cs, S_slab, S_go, hazard)
    go16 = np.zeros((cs.rows, 32), f32)
    go16[:, :4] = hi
    scales = np.array([v for s in list(S_slab) + [S_go] for v in (s, 1.0 / s)], f32)
    gin = None if gin is None else np.stack([cs.unpad(g) for g in gin])
    out = dict(go16=go16, g=stored, scales=scales, gmax=gmax, gin=gin, sat=sat)
    if cs.base is not None:                       # the chain's own scatter: float32 weights, float32 adds onto the base, point by point
        out["gin"], out["vols"] = None, [b.copy() for b in cs.base]
        pts = cs.points[cs.image0:cs.image0 + cs.n_images].reshape(-1, 3)
        for fi, (lvl, cc) in enumerate(cs.feature_tiles()):
            V = cs.levels[lvl][0]
            flat = out["vols"][lvl].reshape(cs.n_images * V ** 3, -1)
            img = np.repeat(np.arange(cs.n_images), cs.npi) * V ** 3
            for idx, w in S.corner_list(pts, V):
                np.add.at(flat[:, cc:cc + 32], img + idx, gin[fi] * w.astype(f32)[:, None])
    return out


# ---- the float64 expectation --------------------------------------------------------------------------------------------------------------
def full_chain64(cs):
    """ga (nslab, rows, H) in true units by the whole chain in float64 from the inputs (no rounding anywhere): for the clamp report."""
    sn, nslab = cs.sn, cs.nslab
    inc = go_prime(cs, F64) @ sn.head_W.astype(F64)
    ga = np.zeros((nslab, cs.rows, sn.H))
    for m in range(nslab - 1, -1, -1):
        if m < nslab - 1:
            inc = (ga[m + 1] * cs.freq_rows(m + 1)) @ sn.mats[m + 1].W.astype(F64)
            if m + 2 < nslab and sn.mats[m + 2].role == "fc2":
                inc = inc + ga[m + 2]
        ga[m] = inc * cs.cos[m].astype(F64)
    return ga


def clamp_report(cs, S_slab):
    """(tile, slab) pairs whose pre-clamp maximum exceeds 65504 (bool (nslab, tiles)), the elements beyond it (bool), and the pre-clamp
    values, and whether every pair is a factor 2 away from the threshold."""
    pre = full_chain64(cs) * np.asarray(S_slab, F64)[:, None, None]
    tmax = np.abs(pre).max(axis=2).reshape(cs.nslab, -1, 32).max(axis=2)
    return tmax > F16_MAX, np.abs(pre) > F16_MAX, pre, bool(((tmax > 2 * F16_MAX) | (tmax < F16_MAX / 2)).all())


def check(cs, out, tag="", strict=True):
    """Every output of one call against float64, each step from the stage's own stored rows.  out: go16 (rows, 32), g (nslab, rows, H)
    stored values, scales, gmax (floats), gin (feature tiles, n, 32) or None, vols [(n_images, V, V, V, C)] or None (pass 2 with a volume:
    the chain added to cs.base itself), sat.  Rows with a clamped element (the sampling case's hot point) are judged by the clamp report.
    Returns {output: worst |err| / bound}; strict = False (the hazard tests): nothing is asserted, the ratios are returned together with
    the equalities that broke under "broken"."""
    sn, nslab, H, rows = cs.sn, cs.nslab, cs.sn.H, cs.rows
    winv, anorm = (t.astype(F64) for t in weight_scales(sn))
    valid = cs.valid
    scales = np.asarray(out["scales"], F64)
    S_slab, S_go = scales[0:2 * nslab:2], scales[2 * nslab]
    gmax = np.asarray(out["gmax"], F64)
    ratios, broken = {}, []

    def claim(cond, *what):
        if strict:
            assert cond, what
        elif not cond:
            broken.append(what[-1] if what and isinstance(what[-1], str) else str(what))

    def held(got, want, bound, what, keep=None):
        got, want, bound = (np.asarray(t, F64) for t in (got, want, bound))
        if keep is not None:
            got, want, bound = got[keep], want[keep], bound[keep]
        if not np.isfinite(got).all() or not got.size:
            claim(False, what + " holds no finite rows")
            return
        if strict:
            within(got, want, bound, tag + what)
        err = np.abs(got - want)
        ratios[what] = max(ratios.get(what, 0.0), float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0)))))

    claim(np.array_equal(scales[1::2], 1.0 / scales[0::2]) and (np.frexp(scales)[0] == 0.5).all(), "scales are {S, 1 / S}, powers of two")
    step = cs.group_step or production_step(cs.n_images, cs.tpi)
    tiles = tiles_of_groups(sampled_groups(cs.n_images, cs.tpi, step), cs.tpi)
    srow = (np.asarray(tiles)[:, None] * 32 + np.arange(32)).reshape(-1)

    # the head's scale: the exact maximum of the chunk's upstream rows
    upmax = float(np.abs(cs.upstream[cs.image0:cs.image0 + cs.n_images]).max())
    claim(gmax[nslab + 1] == upmax and S_go == pow2_scale_rule(upmax), (gmax[nslab + 1], upmax, S_go), "head scale")

    # rows of the hot point's clamped elements are judged by the clamp report, everything else by the bounds
    pairs, beyond, pre, apart = clamp_report(cs, S_slab)
    claim(apart, "a (tile, slab) maximum within a factor 2 of fp16's largest number")
    claim(int(out["sat"]) == int(pairs.sum()), (out["sat"], int(pairs.sum())), "saturated count")
    ok = ~beyond.any(axis=(0, 2))                                       # rows without a clamped element in any slab
    if cs.hot is None:
        claim(ok.all() and not pairs.any(), "only the sampling case may clamp")
    else:
        hot_row = cs.hot[0] * cs.tpi * 32 + cs.hot[1]
        claim((~ok).sum() == 1 and not ok[hot_row], "the hot point's row alone is clamped")
        far = np.abs(pre) > 1.02 * F16_MAX                              # (the whole-chain float64 value is good to ~1e-3)
        claim(far.any() and np.array_equal(np.asarray(out["g"], F64)[far], np.sign(pre[far]) * F16_MAX), "clamped elements are +-65504")

    go = go_prime(cs, F64)
    g16 = np.asarray(out["go16"], F64)
    want = go * S_go
    bound = HF * np.abs(want) + FL
    if sn.sigmoid:
        bound[:, :3] += 3 * U * np.abs(want[:, :3])
    bound[~valid] = 0.0
    claim(np.abs(want).max() < 60000.0)
    held(g16[:, :4], want, bound, "go16")
    claim(not g16[:, 4:].any(), "channels 4..31 of go16 are zero")
    claim(not g16[~valid].any() and not np.asarray(out["g"])[:, ~valid].any(), "rows past an image's end are zero")
    gomax_s = float(np.abs(go[srow]).max())
    claim(abs(gmax[nslab] - gomax_s) <= 3 * U * gomax_s, "sampled maximum of the head gradient")

    gh = np.asarray(out["g"], F64) / S_slab[:, None, None]              # stored rows in true units
    fmax = cs.fmax_rows()
    Wh = sn.head_W.astype(F64)
    dgo = (3 * U + 2.0 ** -22) * np.abs(go) + FL / S_go
    inc = go @ Wh
    dinc = dgo @ np.abs(Wh) + np.abs(go) @ (HF * np.abs(Wh) + FL * winv[nslab]) + dot_bound(8, go.T, Wh)
    T = [None] * nslab
    T[nslab - 1] = pow2_to_2p14(fmax[:, nslab - 1] * anorm[nslab] * np.abs(go).max(axis=1)) / 2.0
    gpmax = [None] * nslab
    for m in range(nslab - 1, -1, -1):
        dident = 0.0
        if m < nslab - 1:
            fr = cs.freq_rows(m + 1)
            gp = gh[m + 1] * fr
            dgp = (2 * HF + 3 * U) * np.abs(gp) + np.abs(fr) * FL / S_slab[m + 1] + (FL / T[m + 1])[:, None]
            W = sn.mats[m + 1].W.astype(F64)
            inc = gp @ W
            dinc = dgp @ np.abs(W) + np.abs(gp) @ (HF * np.abs(W) + FL * winv[m + 1]) + dot_bound(H, gp.T, W)
            skip = m + 2 < nslab and sn.mats[m + 2].role == "fc2"
            if skip:
                ident = gh[m + 2]
                dident = (2 * HF + 3 * U) * np.abs(ident) + FL / S_slab[m + 2] + (FL / T[m + 2])[:, None] + U * np.abs(inc + ident)
                inc = inc + ident
            T[m] = pow2_to_2p14(fmax[:, m] * (anorm[m + 1] * gpmax[m + 1] + (gpmax[m + 2] if skip else 0.0))) / 2.0
        c = cs.cos[m].astype(F64)
        want = inc * c
        pre_b = np.abs(c) * (dinc + dident) + 3 * U * np.abs(want)
        bound = pre_b + HF * np.abs(want) + FL / S_slab[m]
        bound[~valid] = 0.0
        held(gh[m], want, bound, f"g16[{m}] {sn.mats[m].role}", keep=ok)
        gpmax[m] = np.abs(gh[m]).max(axis=1) * fmax[:, m]
        # the slab's scale and sampled maximum (the hot row is never sampled)
        M = float(np.abs(want[srow]).max())
        db = float(pre_b[srow].max())
        claim(ok[srow].all(), "a sampled row is clamped")
        claim(pow2_distance(M) * M > db, (cs.name, m, M, db), "sampled maximum too close to a power of two for the equality of scales")
        claim(S_slab[m] == pow2_scale_rule(M), (cs.name, m, S_slab[m], M), "slab scale")
        claim(abs(gmax[m] - M) <= db, (cs.name, m, gmax[m], M, db), "slab gmax")
        claim(float(f16(gmax[m] * S_slab[m])) >= np.abs(np.asarray(out["g"], F64)[m][srow]).max(), (cs.name, m), "gmax below a stored value")

    tiles_f = cs.feature_tiles()
    if not tiles_f:
        claim(out.get("gin") is None and not out.get("vols"))
        return dict(ratios, broken=broken)
    fr = cs.freq_rows(0)
    gp = gh[0] * fr
    dgp = (2 * HF + 3 * U) * np.abs(gp) + np.abs(fr) * FL / S_slab[0] + (FL / T[0])[:, None]
    W0 = cs.W0_padded(F64)
    all_tiles = S.input_tiles(sn, [np.zeros((1, 1, 1, 1, c)) for _, c in cs.levels])
    want_f, bound_f = [], []
    for tk, (lvl, _) in enumerate(all_tiles):
        if lvl < 0:
            continue
        Wc = W0[:, 32 * tk:32 * tk + 32]
        w_ = gp @ Wc
        b_ = dgp @ np.abs(Wc) + np.abs(gp) @ (HF * np.abs(Wc) + FL * winv[0]) + dot_bound(H, gp.T, Wc) + 3 * U * np.abs(w_)
        want_f.append(cs.unpad(w_))
        bound_f.append(cs.unpad(b_))
    okp = cs.unpad(ok[:, None].astype(F64))[:, 0] > 0
    if out.get("gin") is not None:
        for fi in range(len(tiles_f)):
            claim(np.abs(want_f[fi]).max() > 0)
            held(out["gin"][fi], want_f[fi], bound_f[fi], "gin", keep=okp)
            if cs.copies:                          # per-point scales: the chain of a point times 2^-k is the point's chain times 2^-k, bit for bit
                g = np.asarray(out["gin"][fi], F64).reshape(cs.n_images, cs.npi, 32)
                k = np.arange(cs.npi) % cs.copies
                claim(np.abs(g[:, k == cs.copies - 1]).min(axis=2).max() > 0, "the smallest copies' rows are not zero")
                claim(np.array_equal(g * (2.0 ** k)[None, :, None], g[:, np.arange(cs.npi) - k]), "gin rows of power-of-two copies are exact multiples")
    else:
        claim(cs.hot is None)
        pts = cs.points[cs.image0:cs.image0 + cs.n_images]
        unreachable = 0
        for lvl, (V, C) in enumerate(cs.levels):
            base = cs.base[lvl].astype(F64)
            want_v, bound_v = base.copy(), np.zeros(base.shape)
            for fi, (tl, cc) in enumerate(tiles_f):
                if tl != lvl:
                    continue
                w_, b_ = S.scatter64(want_f[fi].reshape(cs.n_images, cs.npi, 32), bound_f[fi], pts, V, cs.npi)
                want_v[..., cc:cc + 32] += w_
                bound_v[..., cc:cc + 32] = b_ + addend_count(pts, V, cs.npi) * U * np.abs(base[..., cc:cc + 32])
            unreachable += int((bound_v == 0).sum())
            held(out["vols"][lvl], want_v, bound_v, "grad volume")
        claim(unreachable > 0, "some voxels are out of every sample's reach: equality is demanded there")
    return dict(ratios, broken=broken)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
PYRAMID5 = [(8, 64), (4, 32), (3, 64)]          # five feature tiles (odd: the last layer-0 weight unit is half padding), two in a level
ONE_LEVEL = [(8, 32)]

#        name              variant                 H    B  R  S   pass image0 n_images step  kind
CASES = {
    "fg64_coarse":       ("SHORTSIREN_FG",        64,  2, 5, 7,  0, 0, 2, 0, "plain"),
    "fg128_fine":        ("SHORTSIREN_FG",        128, 2, 5, 7,  1, 0, 2, 0, "plain"),
    "fg256_points":      ("SHORTSIREN_FG",        256, 2, 5, 7,  2, 0, 2, 0, "plain"),
    "fg64_image_range":       ("SHORTSIREN_FG",        64,  3, 1, 33, 0, 1, 2, 0, "plain"),
    "fg128_freq64":      ("SHORTSIREN_FG",        128, 2, 5, 7,  0, 0, 2, 0, "freq64"),
    "dgx64_fine":        ("TALLSIREN_dgx",        64,  3, 1, 33, 1, 0, 3, 0, "plain"),
    "dgx256_points":     ("TALLSIREN_dgx",        256, 3, 1, 33, 2, 1, 2, 0, "plain"),
    "pyrmd128_coarse":   ("SHORTSIREN_FG_Pyrmd",  128, 2, 5, 7,  0, 0, 2, 0, "plain"),
    "pyrmd64_points":    ("SHORTSIREN_FG_Pyrmd",  64,  3, 1, 33, 2, 1, 2, 0, "plain"),
    "sine256_coarse":    ("SHORTSIREN_F",         256, 3, 1, 33, 0, 0, 3, 0, "plain"),
    "res64_fine":        ("SHORTSIREN_FRes",      64,  2, 5, 7,  1, 0, 2, 0, "plain"),
    "res256_coarse":     ("SHORTSIREN_FRes",      256, 2, 5, 7,  0, 0, 2, 0, "plain"),
    "res2_128_points":   ("TALLSIREN_dRes",       128, 2, 5, 7,  2, 0, 2, 0, "plain"),
    "novol64_coarse":    ("SHORTSIREN",           64,  2, 5, 7,  0, 0, 2, 0, "plain"),
    "wide128_coarse":    ("SHORTSIREN_FG",        128, 2, 5, 7,  0, 0, 2, 0, "wide"),
    "wide_res64_fine":   ("SHORTSIREN_FRes",      64,  2, 5, 7,  1, 0, 2, 0, "wide"),
    "copies_dres64":     ("TALLSIREN_dRes",       64,  2, 5, 7,  1, 0, 2, 0, "copies"),
    "copies_dgx128":     ("TALLSIREN_dgx",        128, 2, 5, 7,  0, 0, 2, 0, "copies"),
    "sampling_step2":    ("SHORTSIREN_FG",        64,  2, 8, 16, 0, 0, 2, 2, "sampling"),
    "sampling_step1":    ("SHORTSIREN_FG",        64,  2, 8, 16, 0, 0, 2, 1, "sampling"),
}


def make_net(variant, H, seed, levels):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators import siren
    torch.manual_seed(seed)
    cls = getattr(siren, variant)
    C = sum(c for _, c in levels)
    if cls.spec.input == "position":
        return cls(3, Z_DIM, H).eval()
    return cls(input_dim=C + (3 if cls.spec.input == "feat_xyz" else 0), z_dim=C if cls.spec.input_is_zdim else Z_DIM, hidden_dim=H).eval()


def case(name):
    """The inputs of a case: deterministic, the same on every machine (torch's CPU generator, NumPy's PCG64)."""
    import torch
    variant, H, B, R, Sr, pss, image0, n_images, step, kind = CASES[name]
    seed = sum(map(ord, name.split("_step")[0]))        # (the two sampling cases share their inputs)
    rng = np.random.default_rng(seed)
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators import siren
    spec = getattr(siren, variant).spec
    levels = [] if spec.input == "position" else PYRAMID5 if spec.input == "pyramid" else ONE_LEVEL
    net = make_net(variant, H, seed, levels)
    sn = S.stage_net(net)
    npi, tpi = R * R * Sr, (R * R * Sr + 31) // 32
    nslab, rows = len(sn.mats), n_images * tpi * 32
    upstream = rng.standard_normal((B, npi, 4)).astype(f32)
    saved = rng.uniform(0.02, 0.98, (B, npi, 4)).astype(f32)
    freq = None
    if spec.has_global:
        with torch.no_grad():
            freq = net.film(torch.from_numpy(rng.standard_normal((B, Z_DIM)).astype(f32)))[0].numpy().astype(f32)
        if kind == "freq64":                      # image 1's frequencies 2^6 below image 0's
            freq[1] = freq[0] * f32(2.0 ** -6)
    cos = rng.uniform(-1.0, 1.0, (nslab, rows, H)).astype(np.float16)
    special = rng.random((nslab, rows, H))
    cos[special < 0.02] = 1.0
    cos[(special >= 0.02) & (special < 0.04)] = -1.0
    cos[(special >= 0.04) & (special < 0.06)] = 0.0
    hot = None
    if kind == "wide":                            # within every tile the rows span 2^24 in powers of two
        upstream *= (2.0 ** -(np.arange(npi) % 25)).astype(f32)[None, :, None]
    if kind == "copies":                          # ... and each run of 25 points is ONE point (8-bit upstream, its cosines) times 2^0 .. 2^-24
        assert not spec.sigmoid_rgb, "s (1 - s) would give the head operand a low part, which fp16's subnormals cut off for the small copies"
        k = np.arange(npi) % 25
        upstream = (rng.integers(-127, 128, (B, npi, 4)) / 64.0).astype(f32)[:, np.arange(npi) - k] * (2.0 ** -k).astype(f32)[None, :, None]
        src = (np.arange(tpi * 32) - np.where(np.arange(tpi * 32) < npi, np.arange(tpi * 32) % 25, 0))
        cos = cos.reshape(nslab, n_images, tpi * 32, H)[:, :, src].reshape(nslab, rows, H)
    if kind == "sampling":                        # one point of an unsampled group carries 2^20 x the largest upstream gradient
        sampled = set(tiles_of_groups(sampled_groups(n_images, tpi, 2), tpi))
        tile = next(t for t in range(tpi, 2 * tpi) if t not in sampled)          # in image 1 of the chunk
        hot = (1, (tile - tpi) * 32 + 13)
        big = f32(2.0 ** 20) * np.abs(upstream).max()
        upstream[image0 + 1, hot[1]] = np.array([big, -big / 2, big / 4, big], f32)
        if step == 1:
            hot = None                            # every group is sampled: nothing clamps
    points = (rng.standard_normal((B, npi, 3)) * 0.35).astype(f32)
    points[..., 0] = -np.abs(points[..., 0])      # x <= 0: the nodes 6 and 7 of a level of side 8 are out of every sample's reach
    base = None
    if pss == 2 and levels:
        base = [(0.5 * rng.standard_normal((n_images, V, V, V, C))).astype(f32) for V, C in levels]
    return Case(name, sn, levels, B, R, Sr, pss, image0, n_images, step, upstream, saved, freq, cos, points, hot, base, 25 if kind == "copies" else 0), net
