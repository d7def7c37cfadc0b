"""The half-precision gradient chain of the per-point FiLM family (cnerf_field_chain_pw16 -> pwchain::chain_pre_kernel and
pwchain::pw_gm_kernel, csrc/chain_pw16.hip) row by row in float64: the expectation and its derived bound, a float32 NumPy emulation of
the two kernels' arithmetic (honest, or with ONE named hazard), and the cases shared by tests/test_chain_pw16_cpu.py and
tests/test_gpu_chain_pw16.py.  Built like tests/chain16_common.py, whose scalar rules, layouts and sampled-group restatement it imports.

Every check is LAYER-LOCAL: the expectation of a stored row comes from what the stage itself stored one step earlier, in float64.
h = 2^-11 (fp16 unit roundoff), u = 2^-24, FL = 2^-25 (half the spacing of fp16's subnormals).  Per layer l the caller supplies three
derivative rows d = (cos, cos f, cos 15 pre) as fp16, amax = the point's largest |d|, and m16 (only its sign is read).

What the kernels do per point, in the order of chain_pw16.hip
--------------------------------------------------------------
chain_pre   go' = upstream (TALLSIREN has no sigmoid; with one: * s (1 - s)); gs = go' S_go; go16 = fp16(gs); the head operand is
            fp16(gs) + fp16(gs - fp16(gs)).  Layer lam = L-1 .. 0: av = accumulator of head^T operand (two MFMAs, 8 products) or of
            W_{lam+1}^T operand_{lam+1} (fp32 sums of exact fp16 x fp16 products); U = winv / (S_go or T_{lam+1}) un-scales it;
            gy16[lam] = fp16(clamp(av U S_y,lam)); operand_lam = fp16((av cos f) U T), T = pow2_to_2p14(amax ||W||_1 max |g_pre|): per POINT.
pw_gm       per layer: gy = gy16[l] (fp16), the three stored slabs fp16(gy d r_l), the operands fp16(gy d To_l) (not clamped: a point
            of an unsampled group is stored unclamped by chain_pre up to 32 x the sampled maximum, its operand can be +-inf, and chain_pre
            reports that), g_m +=
            Wm2[fr rows]^T ofr + Wm2[ph rows]^T oph in 8 resident accumulator tiles, re-scaled by rho = unit_l / unit_{l-1} at every layer
            boundary (unit_l = S_y,l To_l / winv_l: all powers of two).  Tail: v = g_m / unit LeakyReLU'(m); g_mpre = fp16(clamp(v S_mp));
            operand fp16(v Tm), Tm = pow2_to_2p14(the point's max |v| over BOTH half-rows); g_feat = (Wm1^T operand) winv / Tm in fp32,
            scattered with the trilinear weights by atomics.

Derivations
-----------
go16        as tests/chain16_common.py: (3 u [sigmoid only] + h) |gs| + FL in stored units; channels 4..31 and rows past an image's end: 0.
gy16[L-1]   head^T go' with the hi + lo operand: d go = (3 u + 2^-22) |go| + FL / S_go; the head packed as fp16(W s): h |W| + FL / s per
            weight; 8 product terms in two MFMAs: dot_bound(8); one fp32 product with U S_y (u |want|: a power of two, exact in fact);
            one fp16 store at S_y: h |want| + FL / S_y.  A clamped element is exactly +-65504.
gy16[l]     l < L-1, from the STORED gh = gy16[l+1] / S_y,l+1 and the caller's cos f rows of layer l + 1: gp = gh cos f.  The stored value
            and the MFMA operand are two fp16 conversions of one fp32 accumulator (times cos f: one fp32 rounding):
                |operand / T - gp| <= (2 h + 3 u) |gp| + |cos f| FL / S_y,l+1 + FL / T
            T per point, ONE BINADE BELOW pow2_to_2p14(amax ||W||_1 max |g_pre|) formed from the stored rows, so a knife-edge exponent
            cannot decide a failure.  W_{l+1}^T packed as fp16 with its own power-of-two scale: |gp| (h |W| + FL / s); the sum is an
            fp32 sum of length H in any order: dot_bound(H); the store at S_y,l: (u + h) |want| + FL / S_y,l.
slabs       g16[3 l + s] = fp16(float32(gy16) float32(d16) r_l) BIT FOR BIT (s = 0: cos f, 1: cos 15 pre, 2: cos): both factors are fp16
            values, so their fp32 product is exact (22 bits); r_l is a power of two; one round-to-nearest-even conversion, subnormals
            included.  |d| r_l <= 1 and |gy16| <= 65504: no overflow.
lay, scales r_l = 2^-ceil(log2 max(1, largest amax of layer l over ALL tiles * 32 entries, padded rows included)); To_l = 8 r_l;
            scales[3 l + s] = {S_y,l r_l, 1 / (S_y,l r_l)}.  S_y,l and S_mp = pow2_scales_kernel's rule on the float64 maximum of the
            SAMPLED rows' expectation, asserted only where that maximum sits further from a power of two than the row bound; the sampled
            maxima themselves lie within that bound of it.  gmax[3 L + 1] is the chunk's largest |upstream| (the head's scale).
g_mpre      the operands ofr = fp16(gy16 d_fr To), oph = fp16(gy16 d_ph To) are exactly computable on the host, so
                want = LeakyReLU'(m16) sum_l (Wm2[fr rows of l]^T ofr_l + Wm2[ph rows of l]^T oph_l) / (S_y,l To_l)
            and the bound holds only: the packed weights' rounding (h |W| + FL / s; freq and phase rows of a layer share one s); an fp32
            sum of 2 L H terms in any order: dot_bound(2 L H); the re-scalings by rho, which are exact as long as no partial sum leaves
            fp32's normal range -- partial sums are sums of products >= 2^-48 of fp16 values, so |log2| of every unit ratio <= 60 is
            enough, and that is asserted; 3 u |want| (1 / unit, the slope, whose 0.2f is taken as the float32 it is); one clamped
            fp16 store at S_mp: h |want| + FL / S_mp.  A row with an operand beyond 65504 (the hot points) is judged by `saturated`.
volume      g_feat = Wm1^T g_mpre from the STORED gm^ = g_mpre16 / S_mp: operand fp16(v Tm) and stored fp16(v S_mp) are two conversions
            of one number: 2 h |gm^| + FL / S_mp + FL / Tm, Tm from the point's own maximum over the whole row, one binade low; Wm1^T
            packed: h |W| + FL / s; dot_bound(256); 3 u for the product with winv / Tm; then scatter64's volume terms (fp32 trilinear
            weights, products, any order of the atomics) and k u |base| for a non-zero base.  A voxel out of every sample's reach
            keeps its base bit for bit.
copies      every scale that follows a POINT is a power of two from the point's own maximum, so the chain_pre rows of a point times 2^-k
            are the point's rows times 2^-k bit for bit wherever the stored fp16 is normal (> 2^-14): demanded of the "copies" case.  It
            is what carries an operand scale T per tile: every stored row sits at a call-wide scale S_y whose floor FL / S_y is coarser
            than FL / T of any tile, so no tolerance on a stored row can see it.
saturated   chain_pre: += 1 per (tile, layer) with a point whose g_y S_y exceeds 65504 (clamped), or whose (max |g_y| S_y) amax To_l exceeds
            65472: |gy16| <= |g_y| S_y (1 + h) and |d| <= amax, so below that no operand of pw_gm reaches 65520, where fp16's conversion
            turns to +-inf.  The expectation takes g_y from the whole chain in float64; the cases keep every such product 2 % away from
            its threshold.  The contract "non-zero means: repeat in fp32": every row with an operand beyond 65504 (computable exactly
            from the stored gy16) lies in a counted (tile, layer); such a row's g_mpre and the voxels it reaches are not judged.
            pw_gm: += 1 per tile with a g_mpre beyond 65504 (none in these cases).
padded rows cos16 / m16: +-65504; amax: 0.25, and in the even layers 1.7 x the layer's real maximum, which moves r_l a binade.  An amax of
            3e38 is not among them: pw_split_scales_kernel reads a value >= 3e38 as "no maximum" (r_l = 1), real rows then overflow, and
            no storing forward writes such a value (include/cnerf.h says what the padded rows may hold).
Terms corrected on the hardware: none (see tests/test_gpu_chain_pw16.py for the measured ratios).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import field_backward_stage_common as S
from chain16_common import (F16_MAX, FL, HF, f16, f32, from_tb16, idle_waves, pow2_distance, pow2_scale_rule, pow2_to_2p14,      # noqa: F401
                            pow2_weight_scale, sampled_groups, tiles_of_groups, to_cos16)
from field_backward_stage_common import F64, U, dot_bound, within      # noqa: F401
from scatter_patch_common import Geom, addend_count

SLOPE = float(np.float32(0.2))


def production_step(n_images, tpi):
    """chain_pw16_sequence: groups / 1024, clamped to 1..32."""
    return int(np.clip(n_images * ((tpi + 3) // 4) // 1024, 1, 32))


def to_tb16(rows, CT):
    """rows (tiles * 32, 32 CT) -> TB16 (tiles, CT, 32 points, 32 channels) flat."""
    n = rows.shape[0]
    return np.ascontiguousarray(rows.reshape(n // 32, 32, CT, 32).transpose(0, 2, 1, 3)).reshape(-1)


@dataclass
class Case:
    """One call on the chunk's images.  Arrays hold the chunk only unless they say FULL: rows = n_images * tpi * 32 padded rows."""
    name: str
    sn: S.StageNet
    V: int
    B: int
    R: int
    Sr: int
    pss: int
    image0: int
    n_images: int
    group_step: int
    upstream: np.ndarray                # FULL (B, npi, 4) float32
    saved: np.ndarray                   # FULL (B, npi, 4) float32
    cos: np.ndarray                     # (3 L, rows, H) float16: per layer cos, cos f, cos 15 pre
    amax: np.ndarray                    # (L, rows) float32
    m16: np.ndarray                     # (rows, 256) float16
    cams: np.ndarray                    # FULL (B, 4, 4) float32
    u_strat: np.ndarray                 # FULL (B, npi) float32
    fine_z: np.ndarray                  # FULL (B, npi) float32
    points: np.ndarray                  # FULL (B, npi, 3) float32: pass 2 reads them, the ray passes form their own (= these, by Geom)
    base: np.ndarray                    # (n_images, V, V, V, 32) float32: what the chunk's gradient volume holds before the call
    hot: Optional[tuple] = None         # (image of the chunk, point) of the one huge upstream row
    copies: int = 0

    @property
    def L(self):
        return len(self.sn.mats)

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
    def pts(self):
        return self.points[self.image0:self.image0 + self.n_images]

    def pad(self, t, fill_last=False):
        t = t[self.image0:self.image0 + self.n_images]
        out = np.zeros((self.n_images, self.tpi * 32, t.shape[-1]), t.dtype)
        out[:, :self.npi] = t
        if fill_last:
            out[:, self.npi:] = t[:, -1:]
        return out.reshape(self.rows, -1)

    def unpad(self, rows):
        return rows.reshape(self.n_images, self.tpi * 32, -1)[:, :self.npi].reshape(self.n_images * self.npi, -1)

    def srow(self):
        step = self.group_step or production_step(self.n_images, self.tpi)
        tiles = tiles_of_groups(sampled_groups(self.n_images, self.tpi, step), self.tpi)
        return (np.asarray(tiles)[:, None] * 32 + np.arange(32)).reshape(-1)


def go_prime(cs, dtype, fill_last=False):
    up, so = cs.pad(cs.upstream, fill_last).astype(dtype), cs.pad(cs.saved, fill_last).astype(dtype)
    go = up.copy()
    if cs.sn.sigmoid:
        go[:, :3] = up[:, :3] * (so[:, :3] * (dtype(1.0) - so[:, :3]))
    return go


class Weights:
    """The matrices and the scales launch_pack_pw_chain forms: winv = [W_l^T: L (0 unused) | Wm2 pair of layer l: L | Wm1^T | head^T],
    anorm = [||W_l||_1: L (0 unused) | head]."""

    def __init__(self, sn):
        L, H = len(sn.mats), sn.H
        self.Wm1, _, self.Wm2, _ = sn.map
        self.W = [m.W for m in sn.mats]
        self.head = sn.head_W
        col = lambda W: np.abs(W).astype(f32).sum(axis=0, dtype=f32).max()
        self.winv, self.anorm = np.zeros(2 * L + 2, f32), np.zeros(L + 1, f32)
        for l in range(1, L):
            self.winv[l], self.anorm[l] = 1.0 / pow2_weight_scale(np.abs(self.W[l]).max()), col(self.W[l])
        self.fr = [self.Wm2[l * H:(l + 1) * H] for l in range(L)]                    # (H, 256) each
        self.ph = [self.Wm2[(L + l) * H:(L + l + 1) * H] for l in range(L)]
        for l in range(L):
            self.winv[L + l] = 1.0 / pow2_weight_scale(max(np.abs(self.fr[l]).max(), np.abs(self.ph[l]).max()))
        self.winv[2 * L], self.winv[2 * L + 1] = 1.0 / pow2_weight_scale(np.abs(self.Wm1).max()), 1.0 / pow2_weight_scale(np.abs(self.head).max())
        self.anorm[L] = col(self.head)
        q = lambda W, wi: f16(W * f32(1.0 / wi))
        self.Y16 = [None] + [q(self.W[l], self.winv[l]) for l in range(1, L)]
        self.fr16 = [q(self.fr[l], self.winv[L + l]) for l in range(L)]
        self.ph16 = [q(self.ph[l], self.winv[L + l]) for l in range(L)]
        self.W1_16, self.head16 = q(self.Wm1, self.winv[2 * L]), q(self.head, self.winv[2 * L + 1])


def r_of(amax_layer_max):
    """pw_split_scales_kernel: r = 2^-ceil(log2 max(1, am)) (am outside [1, 3e38): 1)."""
    am = float(amax_layer_max)
    if not (am >= 1.0 and am < 3e38):
        am = 1.0
    m, e = np.frexp(am)
    return float(2.0 ** -(e - 1 if m == 0.5 else e))


# ---- float32 emulation of the two kernels ---------------------------------------------------------------------------------------------
HAZARDS = ("cosf_from_cos15", "row_slot_stale", "gy_prev_layer", "fr_ph_swapped", "rho_skipped", "rho_seven_of_eight", "stale_weight_unit",
           "slope_neighbour_tile", "Tm_half_row", "T_per_tile", "padded_lane_stores", "padded_lane_scatters", "gmax_wrong_slot",
           "operand_range_unreported")


def _site(cs):
    """(layer, channel tile) the single-unit hazards strike: a middle layer, the last tile."""
    return min(cs.L - 1, 3), cs.sn.H // 32 - 1


def _pre32(cs, Wt, S_go, hz):
    """chain_pre on all tiles: fp16(gs) (rows, 4), per layer the accumulator av (rows, H) and its un-scale U (rows), gomax (rows)."""
    L, rows = cs.L, cs.rows
    go = go_prime(cs, f32, hz == "padded_lane_stores")          # `if (!valid) go = 0` forgotten: the padded lane repeats the last point
    gs = np.clip(go * f32(S_go), f32(-60000.0), f32(60000.0))
    hi = f16(gs)
    lo = f16(gs - hi)
    gomax = np.abs(go).max(axis=1)
    z = lo @ Wt.head16 + hi @ Wt.head16
    per_tile = (lambda b: np.repeat(b.reshape(-1, 32).max(axis=1), 32)) if hz == "T_per_tile" else (lambda b: b)
    av, Us = [None] * L, [None] * L
    T_prev = gpm = None
    for lam in range(L - 1, -1, -1):
        first = lam == L - 1
        Uacc = np.full(rows, Wt.winv[2 * L + 1] / f32(S_go), f32) if first else Wt.winv[lam + 1] / T_prev
        T = pow2_to_2p14(per_tile((cs.amax[lam] * (Wt.anorm[L] * gomax if first else Wt.anorm[lam + 1] * gpm)).astype(f32)))
        cf = cs.cos[3 * lam + (2 if hz == "cosf_from_cos15" else 1)].astype(f32)
        vpre = z * cf
        av[lam], Us[lam] = z, Uacc
        op = f16(vpre * (Uacc * T)[:, None])
        gpm = np.abs(vpre).max(axis=1) * Uacc
        T_prev = T
        if lam:
            z = op @ Wt.Y16[lam]
    return hi, av, Us, gomax


def _gm32(cs, Wt, gy, S_y, r, To, hz):
    """pw_gm up to the tail's v = g_m / unit LeakyReLU'(m): the 3 L stored slabs (float32 values of the fp16), v (rows, 256), whether a
    row's operands went beyond 65504 (+-inf: the kernel does not clamp them)."""
    L, H, rows = cs.L, cs.sn.H, cs.rows
    NT = H // 32
    l0, t0 = _site(cs)
    gm = np.zeros((rows, 256), f32)
    slabs = np.zeros((3 * L, rows, H), f32)
    over = np.zeros(rows, bool)
    unit_prev = f32(1.0)
    for l in range(L):
        unit = f32(S_y[l]) * f32(To[l]) / Wt.winv[L + l]
        rho, unit_prev = (f32(1.0) if l == 0 else unit / unit_prev), unit
        g = gy[l - 1] if hz == "gy_prev_layer" and l == l0 and l else gy[l]
        c = [cs.cos[3 * l + s].astype(f32) for s in range(3)]
        if hz == "row_slot_stale" and l == l0 and l * NT + t0 >= 2:          # the prefetch slot still holds the rows of two tiles before
            l2, t2 = divmod(l * NT + t0 - 2, NT)
            for s in range(3):
                c[s] = c[s].copy()
                c[s][:, 32 * t0:32 * t0 + 32] = cs.cos[3 * l2 + s][:, 32 * t2:32 * t2 + 32].astype(f32)
        vph, vpre, vfr = g * c[0], g * c[1], g * c[2]
        slabs[3 * l], slabs[3 * l + 1], slabs[3 * l + 2] = f16(vpre * f32(r[l])), f16(vfr * f32(r[l])), f16(vph * f32(r[l]))
        ofr, oph = vfr * f32(To[l]), vph * f32(To[l])
        over |= (np.maximum(np.abs(ofr), np.abs(oph)) > F16_MAX).any(axis=1)
        ofr, oph = f16(ofr), f16(oph)
        Wf, Wp = Wt.fr16[l], Wt.ph16[l]
        ts = slice(32 * t0, 32 * t0 + 32)
        if l == l0 and hz == "fr_ph_swapped":                                 # the unit's freq and phase k-chunks the other way round
            Wf, Wp = Wf.copy(), Wp.copy()
            Wf[ts], Wp[ts] = Wt.ph16[l][ts], Wt.fr16[l][ts]
        if l == l0 and hz == "stale_weight_unit":                            # the ring slot still holds the unit before
            l2, t2 = divmod(l * NT + t0 - 1, NT)
            Wf, Wp = Wf.copy(), Wp.copy()
            Wf[ts], Wp[ts] = Wt.fr16[l2][32 * t2:32 * t2 + 32], Wt.ph16[l2][32 * t2:32 * t2 + 32]
        if l and not (hz == "rho_skipped" and l == l0):
            if hz == "rho_seven_of_eight" and l == l0:
                gm[:, :224] *= rho
            else:
                gm *= rho
        gm = gm + (ofr @ Wf + oph @ Wp)
    m = cs.m16.astype(f32)
    if hz == "slope_neighbour_tile":
        m = np.roll(m, -32, axis=1)
    v = (gm * (f32(1.0) / unit_prev)) * np.where(m > 0, f32(1.0), f32(0.2))
    return slabs, v, over


def emulate(cs, hazard=None):
    """The stage's outputs (the dict check() reads) from a float32 emulation of the whole sequence."""
    assert hazard is None or hazard in HAZARDS
    with np.errstate(all="ignore"):
        return _emulate(cs, hazard)


def _emulate(cs, hz):
    L, H, rows = cs.L, cs.sn.H, cs.rows
    Wt = Weights(cs.sn)
    srow = cs.srow()
    upmax = float(np.abs(cs.upstream[cs.image0:cs.image0 + cs.n_images]).max())
    S_go = pow2_scale_rule(upmax)
    gmax = np.zeros(5 * L + 2, f32)
    gmax[3 * L + 1] = upmax
    hi, av, Us, _ = _pre32(cs, Wt, S_go, hz)
    my = [np.abs(av[l]).max(axis=1) for l in range(L)]
    ymax = np.array([(my[l] * Us[l])[srow].max() for l in range(L)], f32)
    if hz == "gmax_wrong_slot":                    # the maximum of layer l lands in the slot of layer l + 1
        ymax = np.roll(ymax, 1)
    gmax[3 * L + 2:4 * L + 2] = ymax
    S_y = np.array([pow2_scale_rule(g) for g in ymax])
    gmax[4 * L + 2:] = cs.amax.max(axis=1)
    r = np.array([r_of(a) for a in gmax[4 * L + 2:]])
    To = 8.0 * r
    gy = np.zeros((L, rows, H), f32)
    sat = 0
    for l in range(L):
        USy = Us[l] * f32(S_y[l])
        gy[l] = f16(np.clip(av[l] * USy[:, None], f32(-F16_MAX), f32(F16_MAX)))
        flag = my[l] * USy > F16_MAX
        if hz != "operand_range_unreported":       # chain_pre_kernel before it looked at the range of pw_gm's operands
            flag = flag | ((my[l] * USy) * (cs.amax[l] * f32(To[l])) > f32(65472.0))
        sat += int(flag.reshape(-1, 32).any(axis=1).sum())
    slabs, v, over = _gm32(cs, Wt, gy, S_y, r, To, hz)
    mx = np.fmax.reduce(np.abs(v), axis=1, initial=0.0)                  # fmaxf drops a NaN
    gmax[3 * L] = mx[srow].max()
    S_mp = pow2_scale_rule(gmax[3 * L])
    gmp = f16(np.clip(v * f32(S_mp), f32(-F16_MAX), f32(F16_MAX)))
    sat += int((mx * f32(S_mp) > F16_MAX).reshape(-1, 32).any(axis=1).sum())
    if hz == "Tm_half_row":                        # the h-shuffle of mx dropped: each half-row (channels 8 g + 4 h + e) scales by its own maximum
        half = (np.arange(256) % 8 >= 4)
        mxh = np.stack([np.fmax.reduce(np.abs(v[:, ~half]), axis=1, initial=0.0), np.fmax.reduce(np.abs(v[:, half]), axis=1, initial=0.0)], 1)
        Tm_in, Tm_out = pow2_to_2p14(mxh)[:, half.astype(int)], pow2_to_2p14(mxh)[:, (np.arange(32) % 8 >= 4).astype(int)]
    else:
        Tm_in = Tm_out = pow2_to_2p14(mx)[:, None]
    gfeat = (f16(v * Tm_in) @ Wt.W1_16) * (Wt.winv[2 * L] / Tm_out)
    go16 = np.zeros((rows, 32), f32)
    go16[:, :4] = hi
    sc = list(np.repeat(S_y * r, 3)) + [S_mp, S_go] + list(S_y)
    scales = np.array([x for s in sc for x in (s, 1.0 / s)] + [x for l in range(L) for x in (r[l], To[l])], f32)
    vols = cs.base.copy()
    flat = vols.reshape(cs.n_images * cs.V ** 3, 32)
    img = np.repeat(np.arange(cs.n_images), cs.npi) * cs.V ** 3
    g = cs.unpad(gfeat)
    if hz == "padded_lane_scatters":               # the padded lanes of an image's last tile carry its last point, weight and all
        g = g.reshape(cs.n_images, cs.npi, 32).copy()
        g[:, -1] *= f32(1 + cs.tpi * 32 - cs.npi)
        g = g.reshape(-1, 32)
    for idx, w in S.corner_list(cs.pts.reshape(-1, 3), cs.V):
        np.add.at(flat, img + idx, g * w.astype(f32)[:, None])
    return dict(go16=go16, gy=gy, g=slabs, gmp=gmp, scales=scales, gmax=gmax, vols=vols, sat=sat)


# ---- the float64 expectation ----------------------------------------------------------------------------------------------------------
def full_chain64(cs):
    """Everything by the whole chain in float64 from the inputs, no rounding anywhere: g_y (L, rows, H), g_mpre (rows, 256), g_feat
    (rows, 32), true units."""
    L, H = cs.L, cs.sn.H
    Wt = Weights(cs.sn)
    c = cs.cos.astype(F64)
    inc = go_prime(cs, F64) @ Wt.head.astype(F64)
    gy = np.zeros((L, cs.rows, H))
    gm = np.zeros((cs.rows, 256))
    for l in range(L - 1, -1, -1):
        gy[l] = inc
        gm += (gy[l] * c[3 * l + 2]) @ Wt.fr[l].astype(F64) + (gy[l] * c[3 * l]) @ Wt.ph[l].astype(F64)
        if l:
            inc = (gy[l] * c[3 * l + 1]) @ Wt.W[l].astype(F64)
    gmp = gm * np.where(cs.m16.astype(F64) > 0, 1.0, SLOPE)
    gmp[~cs.valid] = 0.0
    return gy, gmp, gmp @ Wt.Wm1.astype(F64)


def whole_chain_rel_l2(cs, vols):
    """Relative L2 of the stage's volume gradient (its addition to the base) against the float64 chain run end to end."""
    gfeat = full_chain64(cs)[2]
    want, _ = S.scatter64(cs.unpad(gfeat).reshape(cs.n_images, cs.npi, 32), np.zeros((cs.n_images * cs.npi, 32)), cs.pts, cs.V, cs.npi)
    got = np.asarray(vols, F64) - cs.base.astype(F64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def small_point_report(cs, gmp, S_mp):
    """{10: e, 20: e}: the largest error of a stored g_mpre row relative to the POINT's own magnitude, over the points whose magnitude is
    2^-10 / 2^-20 (within a factor 2) of the largest point's.  Reported, not asserted."""
    want = full_chain64(cs)[1]
    mag = np.abs(want).max(axis=1)
    err = np.abs(np.asarray(gmp, F64) / S_mp - want).max(axis=1)
    out = {}
    for k in (10, 20):
        sel = cs.valid & (mag > 0) & (np.abs(np.log2(np.maximum(mag, 1e-300) / mag.max()) + k) <= 1.0)
        out[k] = float((err[sel] / mag[sel]).max()) if sel.any() else float("nan")
    return out


def check(cs, out, tag="", strict=True):
    """Every output of one call against float64, each step from the stage's own stored rows.  out: go16 (rows, 32), gy (L, rows, H), g
    (3 L, rows, H), gmp (rows, 256) stored values, scales, gmax (floats), vols (n_images, V, V, V, 32), sat.  Returns {output: worst
    |err| / bound}; strict = False (the hazard tests): nothing is asserted, the broken equalities are returned under "broken"."""
    L, H, rows, V = cs.L, cs.sn.H, cs.rows, cs.V
    Wt = Weights(cs.sn)
    winv, anorm = Wt.winv.astype(F64), Wt.anorm.astype(F64)
    valid, srow = cs.valid, cs.srow()
    scales = np.asarray(out["scales"], F64)
    gmax = np.asarray(out["gmax"], F64)
    ratios, broken = {}, []

    def claim(cond, *what):
        if strict:
            assert cond, (cs.name,) + what
        elif not cond:
            broken.append(what[-1] if what and isinstance(what[-1], str) else str(what))

    def held(got, want, bound, what, keep=None):
        got, want, bound = (np.asarray(t, F64) for t in (got, want, bound))
        if keep is not None:
            got, want, bound = got[keep], want[keep], bound[keep]
        if not np.isfinite(got).all() or not got.size:
            claim(False, what + " holds a NaN or an infinity")
            ratios[what] = np.inf
            return
        if strict:
            within(got, want, bound, tag + what)
        err = np.abs(got - want)
        ratios[what] = max(ratios.get(what, 0.0), float(np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0)))))

    n_pairs = 4 * L + 2
    pairs = scales[:2 * n_pairs]
    claim(np.array_equal(pairs[1::2], 1.0 / pairs[0::2]) and (np.frexp(pairs)[0] == 0.5).all(), "scales are {S, 1 / S}, powers of two")
    S_of = lambda k: scales[2 * k]
    S_mp, S_go = S_of(3 * L), S_of(3 * L + 1)
    S_y = np.array([S_of(3 * L + 2 + l) for l in range(L)])
    r, To = scales[2 * n_pairs::2], scales[2 * n_pairs + 1::2]
    for l in range(L):
        am = float(cs.amax[l].max())
        claim(gmax[4 * L + 2 + l] == am and r[l] == r_of(am) and To[l] == 8.0 * r[l], (l, r[l], am), "lay: r_l, To_l")
        claim(all(S_of(3 * l + s) == S_y[l] * r[l] for s in range(3)), (l,), "slab scales are S_y r_l")
    claim(not gmax[:3 * L].any(), "unused gmax slots are zero")
    units = S_y * To / winv[L:2 * L]
    claim(np.abs(np.log2(units / units[0])).max() <= 60 and np.abs(np.log2(units)).max() <= 60, "unit ratios within 2^+-60: the re-scalings are exact")
    upmax = float(np.abs(cs.upstream[cs.image0:cs.image0 + cs.n_images]).max())
    claim(gmax[3 * L + 1] == upmax and S_go == pow2_scale_rule(upmax), (gmax[3 * L + 1], upmax, S_go), "head scale")

    # chain_pre's clamp report from the whole chain in float64
    gy64, _, _ = full_chain64(cs)
    pre = gy64 * S_y[:, None, None]
    tmax = np.abs(pre).max(axis=2).reshape(L, -1, 32).max(axis=2)
    beyond = np.abs(pre) > F16_MAX
    claim(bool(((tmax > 2 * F16_MAX) | (tmax < F16_MAX / 2)).all()), "a (tile, layer) maximum within a factor 2 of fp16's largest number")
    opmax = np.abs(pre).max(axis=2) * cs.amax.astype(F64) * To[:, None]            # (L, rows): bound on the point's operands of pw_gm
    claim(bool((np.abs(opmax / 65472.0 - 1.0) > 0.02).all()), "an operand bound within 2 % of its threshold")
    counted = ((np.abs(pre).max(axis=2) > F16_MAX) | (opmax > 65472.0)).reshape(L, -1, 32).any(axis=2)      # (L, tiles)
    ok = ~beyond.any(axis=(0, 2))
    gyst = np.asarray(out["gy"], F64)
    if cs.hot is None:
        claim(ok.all(), "only a hot point may clamp")
    else:
        hot_row = cs.hot[0] * cs.tpi * 32 + cs.hot[1]
        claim(ok[np.arange(rows) != hot_row].all(), "the hot point's row alone may clamp")
        far = np.abs(pre) > 1.02 * F16_MAX
        claim(np.array_equal(gyst[far], np.sign(pre[far]) * F16_MAX), "clamped elements are +-65504")

    go = go_prime(cs, F64)
    g16 = np.asarray(out["go16"], F64)
    want = go * S_go
    bound = HF * np.abs(want) + FL
    if cs.sn.sigmoid:
        bound[:, :3] += 3 * U * np.abs(want[:, :3])
    bound[~valid] = 0.0
    claim(np.abs(want).max() < 60000.0)
    held(g16[:, :4], want, bound, "go16")
    claim(not g16[:, 4:].any(), "channels 4..31 of go16 are zero")
    gst, gmp_st = np.asarray(out["g"], F64), np.asarray(out["gmp"], F64)
    claim(not g16[~valid].any() and not gyst[:, ~valid].any() and not gst[:, ~valid].any() and not gmp_st[~valid].any(), "rows past an image's end are zero")

    # ---- g_y, layer by layer from the stored rows
    gh = gyst / S_y[:, None, None]
    cos = cs.cos.astype(F64)
    Wh = Wt.head.astype(F64)
    dgo = (3 * U + 2.0 ** -22) * np.abs(go) + FL / S_go
    inc = go @ Wh
    dinc = dgo @ np.abs(Wh) + np.abs(go) @ (HF * np.abs(Wh) + FL * winv[2 * L + 1]) + dot_bound(8, go.T, Wh)
    T = pow2_to_2p14(cs.amax[L - 1].astype(F64) * anorm[L] * np.abs(go).max(axis=1)) / 2.0
    for l in range(L - 1, -1, -1):
        if l < L - 1:
            cf = cos[3 * (l + 1) + 1]
            gp = gh[l + 1] * cf
            dgp = (2 * HF + 3 * U) * np.abs(gp) + np.abs(cf) * FL / S_y[l + 1] + (FL / T)[:, None]
            W = Wt.W[l + 1].astype(F64)
            inc = gp @ W
            dinc = dgp @ np.abs(W) + np.abs(gp) @ (HF * np.abs(W) + FL * winv[l + 1]) + dot_bound(H, gp.T, W)
            T = pow2_to_2p14(cs.amax[l].astype(F64) * anorm[l + 1] * np.abs(gp).max(axis=1)) / 2.0
        want = inc
        pre_b = dinc + U * np.abs(want)
        bound = pre_b + HF * np.abs(want) + FL / S_y[l]
        bound[~valid] = 0.0
        held(gh[l], want, bound, f"gy16[{l}]", keep=ok)
        M, db = float(np.abs(want[srow]).max()), float(pre_b[srow].max())
        claim(ok[srow].all(), "a sampled row is clamped")
        claim(abs(gmax[3 * L + 2 + l] - M) <= db, (l, gmax[3 * L + 2 + l], M, db), "sampled maximum of g_y")
        if pow2_distance(M) * M > db:
            claim(S_y[l] == pow2_scale_rule(M), (l, S_y[l], M), "g_y scale")
        claim(float(f16(gmax[3 * L + 2 + l] * S_y[l])) >= np.abs(gyst[l][srow]).max(), (l,), "gmax below a stored value")
        if cs.copies:                              # per-point scales: the rows of a point times 2^-k are the point's rows times 2^-k where normal
            k = np.tile(np.where(np.arange(cs.tpi * 32) < cs.npi, np.arange(cs.tpi * 32) % cs.copies, 0), cs.n_images)
            normal = np.abs(gyst[l]) > 2.0 ** -14      # (2^-14 itself may be a subnormal rounded up)
            claim((normal & (k >= cs.copies - 3)[:, None]).any(), "the smallest copies still hold normal fp16 values")
            claim(np.array_equal(np.where(normal, gyst[l] * (2.0 ** k)[:, None], 0.0), np.where(normal, gyst[l][np.arange(rows) - k], 0.0)),
                  "g_y rows of power-of-two copies are exact multiples")

    # ---- the three stored slabs of every layer: bit for bit; the operands of the mapping products, exactly
    gy32 = np.asarray(out["gy"], f32)
    acc, wterm, absum = np.zeros((rows, 256)), np.zeros((rows, 256)), np.zeros((rows, 256))
    over = np.zeros(rows, bool)
    unreported = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for l in range(L):
            d = [cs.cos[3 * l + s].astype(f32) for s in (1, 2, 0)]              # slab order: g_pre (cos f), g_fr (cos 15 pre), g_ph (cos)
            for s in range(3):
                want16 = ((gy32[l] * d[s]) * f32(r[l])).astype(np.float16)
                got16 = np.asarray(out["g"][3 * l + s], f32).astype(np.float16)
                same = want16.view(np.uint16) == got16.view(np.uint16)
                claim(bool(same.all()), (l, s, int((~same).sum())), "the stored slabs are fp16(gy16 d16 r_l) bit for bit")
            ofr32, oph32 = (gy32[l] * d[1]) * f32(To[l]), (gy32[l] * d[2]) * f32(To[l])
            over_l = (np.maximum(np.abs(ofr32), np.abs(oph32)) > F16_MAX).any(axis=1)
            unreported += int((over_l.reshape(-1, 32).any(axis=1) & ~counted[l]).sum())
            over |= over_l
            ofr, oph = (f16(np.clip(t, -F16_MAX, F16_MAX)).astype(F64) for t in (ofr32, oph32))      # (the clip: rows not judged)
            k = 1.0 / (S_y[l] * To[l])
            Wf, Wp = Wt.fr[l].astype(F64), Wt.ph[l].astype(F64)
            acc += (ofr @ Wf + oph @ Wp) * k
            wterm += (np.abs(ofr) @ (HF * np.abs(Wf) + FL * winv[L + l]) + np.abs(oph) @ (HF * np.abs(Wp) + FL * winv[L + l])) * k
            absum += (np.abs(ofr) @ np.abs(Wf) + np.abs(oph) @ np.abs(Wp)) * k
    okm = ok & ~over
    if cs.hot is None:
        claim(not over.any(), "only a hot point's operands may leave fp16's range")
    else:
        claim(not over[np.arange(rows) != hot_row].any(), "the hot point's operands alone may leave fp16's range")
    slope = np.where(cs.m16.astype(F64) > 0, 1.0, SLOPE)
    want = slope * acc
    pre_b = slope * (wterm + (2 * L * H + 2) * U * absum) + 3 * U * np.abs(want)
    bound = pre_b + HF * np.abs(want) + FL / S_mp
    bound[~valid] = 0.0
    claim(float((np.abs(want[okm]) * S_mp).max()) < F16_MAX / 2, "a g_mpre of an ordinary row near fp16's largest number")
    held(gmp_st / S_mp, want, bound, "g_mpre", keep=okm)
    sm = srow[okm[srow]]
    M, db = float(np.abs(want[sm]).max()), float(pre_b[sm].max())
    claim(okm[srow].all(), "a sampled row left fp16's range")
    claim(abs(gmax[3 * L] - M) <= db, (gmax[3 * L], M, db), "sampled maximum of g_mpre")
    if pow2_distance(M) * M > db:
        claim(S_mp == pow2_scale_rule(M), (S_mp, M), "g_mpre scale")

    # ---- saturated: chain_pre's (tile, layer) pairs; the contract: a row that is not finite and in bound is reported
    claim(unreported == 0, (unreported,), "an operand beyond fp16's range in a (tile, layer) the float64 count does not hold")
    claim(int(out["sat"]) == int(counted.sum()), (int(out["sat"]), int(counted.sum())), "saturated count")
    claim(bool(okm.all()) or int(out["sat"]) > 0, "the contract: outputs finite and in bound, or saturated > 0")

    # ---- the volume: g_feat = Wm1^T g_mpre from the stored rows, scattered
    gmh = np.where(okm[:, None], gmp_st / S_mp, 0.0)
    W1 = Wt.Wm1.astype(F64)
    Tm = pow2_to_2p14(np.abs(gmh).max(axis=1)) / 2.0
    want_f = gmh @ W1
    dg = 2 * HF * np.abs(gmh) + np.where(okm & valid, FL / S_mp + FL / Tm, 0.0)[:, None]
    bound_f = dg @ np.abs(W1) + np.abs(gmh) @ (HF * np.abs(W1) + FL * winv[2 * L]) + dot_bound(256, gmh.T, W1) + 3 * U * np.abs(want_f)
    pts = cs.pts
    w_, b_ = S.scatter64(cs.unpad(want_f).reshape(cs.n_images, cs.npi, 32), cs.unpad(bound_f), pts, V, cs.npi)
    base = cs.base.astype(F64)
    want_v, bound_v = base + w_, b_ + addend_count(pts, V, cs.npi) * U * np.abs(base)
    keep = np.ones(base.shape, bool)
    if not okm[valid].all():                       # the voxels a hot point can reach are its own affair
        cell = np.zeros((cs.n_images * V ** 3, 32))
        i0 = S.corners64(pts.reshape(-1, 3), V)[0]
        bad = ~cs.unpad(okm[:, None].astype(F64))[:, 0].astype(bool)
        np.add.at(cell, (np.repeat(np.arange(cs.n_images), cs.npi) * V ** 3 + (i0[:, 2] * V + i0[:, 1]) * V + i0[:, 0])[bad], 1.0)
        keep = S.nbr_spread(cell.reshape(cs.n_images, V, V, V, 32)) == 0
    held(out["vols"], want_v, bound_v, "grad volume", keep=keep)
    if cs.pss == 2:
        claim(int((bound_v == 0).sum()) > 0, "some voxels are out of every sample's reach: equality is demanded there")
    return dict(ratios, broken=broken)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
V_SIDE = 9
#        name                  H    L  B  R  S   pass image0 n_images step  kind
CASES = {
    "pw64_coarse":          (64,  8, 2, 5, 7,  0, 0, 2, 0, "plain"),
    "pw128_fine":           (128, 8, 2, 5, 7,  1, 0, 2, 0, "plain"),
    "pw256_points":         (256, 8, 2, 5, 7,  2, 0, 2, 0, "base"),
    "pw64_image_range":     (64,  8, 3, 1, 33, 0, 1, 2, 0, "base"),
    "pw128_points_tail1":   (128, 8, 2, 1, 33, 2, 0, 2, 0, "plain"),
    "shallow2_64_points":   (64,  2, 2, 5, 7,  2, 0, 2, 0, "plain"),
    "shallow1_64_fine":     (64,  1, 2, 1, 33, 1, 0, 2, 0, "plain"),
    "wide128_coarse":       (128, 8, 2, 5, 7,  0, 0, 2, 0, "wide"),
    "wide64_points":        (64,  8, 2, 5, 7,  2, 0, 2, 0, "wide"),
    "copies64_fine":        (64,  8, 2, 5, 7,  1, 0, 2, 0, "copies"),
    "sampling_step2":       (64,  8, 2, 8, 16, 0, 0, 2, 2, "sampling"),
    "sampling_step1":       (64,  8, 2, 8, 16, 0, 0, 2, 1, "sampling"),
    "intermediate_step2":   (64,  8, 2, 8, 16, 0, 0, 2, 2, "intermediate"),
}
WHOLE_CHAIN = ("pw64_coarse", "pw128_fine", "pw256_points")
N_COPIES = 19


def make_net(H, L, seed, wide=False):
    """TALLSIREN, or a test-local subclass of it with L layers (check_cfg admits 1 .. CNERF_MAX_LAYERS per-point FiLM layers)."""
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators import siren

    torch.manual_seed(seed)
    if L == 8:
        net = siren.TALLSIREN(3, 32, H).eval()
    else:
        class Shallow(siren.TALLSIREN):
            spec = siren.FieldSpec(("pfilm",) * L, 25, False, False, False, "xyz")

            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.network = torch.nn.ModuleList(list(self.network)[:L])
                self.mapping_network = siren.PointFeaturesMappingNetwork(self.z_dim, 256, L * self.hidden_dim * 2)

        net = Shallow(3, 32, H).eval()
    if wide:                                       # consecutive layers' g_y about 2^+-6 apart: rho and the per-layer scales far from 1
        with torch.no_grad():
            for l in range(1, L):
                net.network[l].layer.weight *= 2.0 ** (6 if l % 2 else -6)
    return net


def _cameras(rng, B):
    """cam2world (B, 4, 4) float32 of cameras on shells r in [0.7, 1.5] looking at the origin, from the case's own generator
    (sample_camera_positions draws from NumPy's global one)."""
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix
    theta = np.clip(np.arccos(1 - rng.random(B)), 1e-5, np.pi - 1e-5)
    phi, r = rng.random(B) * np.pi * 2, rng.random(B) * 0.8 + 0.7
    origin = np.stack([r * np.sin(theta) * np.cos(phi), r * np.cos(theta), r * np.sin(theta) * np.sin(phi)], 1)
    return create_cam2world_matrix(torch.from_numpy(origin).type(torch.float32), "y").numpy().astype(f32)


def case(name):
    """The inputs of a case: deterministic, the same on every machine (torch's CPU generator, NumPy's PCG64)."""
    H, L, B, R, Sr, pss, image0, n_images, step, kind = CASES[name]
    seed = sum(map(ord, name.split("_step")[0])) if kind == "sampling" else sum(map(ord, name))
    rng = np.random.default_rng(seed)
    net = make_net(H, L, seed, kind == "wide")
    sn = S.stage_net(net)
    npi, tpi = R * R * Sr, (R * R * Sr + 31) // 32
    rows = n_images * tpi * 32
    upstream = rng.standard_normal((B, npi, 4)).astype(f32)
    saved = rng.uniform(0.02, 0.98, (B, npi, 4)).astype(f32)
    # the derivative rows: |cos| <= 1, |cos f| up to 40, |cos 15 pre| up to 20, with exact 0 and +-1 among them
    cos = rng.uniform(-1.0, 1.0, (3 * L, rows, H))
    cos[1::3] *= 40.0
    cos[2::3] *= 20.0
    cos = cos.astype(np.float16)
    special = rng.random((3 * L, rows, H))
    cos[special < 0.02] = 1.0
    cos[(special >= 0.02) & (special < 0.04)] = -1.0
    cos[(special >= 0.04) & (special < 0.06)] = 0.0
    m16 = rng.standard_normal((rows, 256)).astype(np.float16)
    m16[rng.random((rows, 256)) < 0.05] = 0.0
    hot, copies = None, 0
    valid = np.tile(np.arange(tpi * 32) < npi, n_images)
    if kind == "wide":                            # within every tile the rows span 2^20 in powers of two
        upstream *= (2.0 ** -(np.arange(npi) % 21)).astype(f32)[None, :, None]
    if kind == "copies":                          # each run of N_COPIES points is ONE point (8-bit upstream, its rows) times 2^0 .. 2^-(N_COPIES - 1)
        copies = N_COPIES
        k = np.arange(npi) % copies
        upstream = (rng.integers(-127, 128, (B, npi, 4)) / 64.0).astype(f32)[:, np.arange(npi) - k] * (2.0 ** -k).astype(f32)[None, :, None]
        src = np.arange(tpi * 32) - np.where(np.arange(tpi * 32) < npi, np.arange(tpi * 32) % copies, 0)
        cos = cos.reshape(3 * L, n_images, tpi * 32, H)[:, :, src].reshape(3 * L, rows, H)
    if kind in ("sampling", "intermediate"):      # one point of an unsampled group of image 1 of the chunk
        sampled = set(tiles_of_groups(sampled_groups(n_images, tpi, 2), tpi))
        tile = next(t for t in range(tpi, 2 * tpi) if t not in sampled)
        hot = (1, (tile - tpi) * 32 + 13)
        hot_row = tile * 32 + 13
    if kind == "sampling":                        # ... carries 2^20 x the largest upstream gradient
        big = f32(2.0 ** 20) * np.abs(upstream).max()
        upstream[image0 + 1, hot[1]] = np.array([big, -big / 2, big / 4, big], f32)
        if step == 1:
            hot = None                            # every group is sampled: nothing clamps
    if kind == "intermediate":
        # ... has a g_y of the last layer 15.9 x the sampled maximum's binade -- stored unclamped, below 2^15 -- in every second channel or so (its
        # upstream has one component: g_y is a row of the head), no g_y below (cos f = 0), and a cos 15 pre row at +- the layer's
        # largest (20; r_l = 1 / 64 from cos f): operands gy16 d To = 2.5 gy16 up to 81000, +-inf in fp16 in every fifth channel or so
        D = np.abs(cos[3 * (L - 1) + 2].astype(F64)).max()
        cos[3 * (L - 1) + 1, hot_row] = 0.0
        cos[3 * (L - 1) + 2, hot_row] = (D * (-1.0) ** np.arange(H)).astype(np.float16)
        cos[3 * (L - 1), hot_row] = ((-1.0) ** (np.arange(H) // 2)).astype(np.float16)
        upstream[image0 + 1, hot[1]] = 0.0
    # padded rows hold large finite values of their own; amax's enter the layer maximum r_l comes from
    cos[:, ~valid] = np.where(rng.random((3 * L, int((~valid).sum()), H)) < 0.5, 65504.0, -65504.0).astype(np.float16)
    cos[1::3, ~valid] = np.float16(-65504.0)
    m16[~valid] = np.where(rng.random((int((~valid).sum()), 256)) < 0.5, 65504.0, -65504.0).astype(np.float16)
    amax = np.stack([np.abs(cos[3 * l:3 * l + 3].astype(f32)).max(axis=0).max(axis=1) for l in range(L)])
    amax[:, ~valid] = f32(0.25)
    amax[0::2, ~valid] = (amax[0::2][:, valid].max(axis=1) * f32(1.7))[:, None]       # beyond the next power of two: r_l is a binade lower for it
    cams = _cameras(rng, B)
    u_strat = rng.random((B, npi)).astype(f32)
    fine_z = (0.25 + 1.7 * rng.random((B, npi))).astype(f32)
    points = (rng.standard_normal((B, npi, 3)) * 0.35).astype(f32)
    points[..., 0] = -np.abs(points[..., 0])      # x <= 0: the nodes of the far side are out of every sample's reach
    if pss != 2:
        geom = Geom(R, Sr)
        points = np.stack([geom.positions(pss, cams[b], (u_strat if pss == 0 else fine_z)[b], np.arange(npi)) for b in range(B)]).astype(f32)
    base = np.zeros((n_images, V_SIDE, V_SIDE, V_SIDE, 32), f32)
    if kind == "base":
        base = (0.5 * rng.standard_normal(base.shape)).astype(f32)
    cs = Case(name, sn, V_SIDE, B, R, Sr, pss, image0, n_images, step, upstream, saved, cos, amax, m16, cams, u_strat, fine_z, points, base, hot, copies)
    if kind == "intermediate":
        Wh = sn.head_W.astype(F64)
        M = 2.0 ** np.ceil(np.log2(np.abs(go_prime(cs, F64)[cs.srow()] @ Wh).max()))      # the sampled maximum's binade: 2048 in stored units
        cs.upstream[image0 + 1, hot[1], 0] = f32(15.9 * M / np.abs(Wh[0]).max())
    return cs, net
