"""The float64 formulas and bounds of tests/field_backward_stage_common.py (what tests/test_gpu_field_backward_stage.py holds the HIP
stage to) against a plain float32 torch emulation of the stage, no GPU.  The emulation is written from the comments of include/cnerf.h:
F.grid_sample for the lookup, F.linear / torch.sin / torch.cos for the rows, matmuls for the transposed products, index_add_ for the
scatter, everything in float32.

1. An honest float32 implementation stays inside every bound: the bounds are attainable.  The emulation's arithmetic differs from the
   kernels' in the order of its sums (any order is inside dot_bound and the volume's reordering term), in ATen's sine and cosine (below
   1 ulp of a value <= 1, 6e-8: inside the polynomials' 1.2e-7 / 1.5e-7) and in ATen's unnormalised coordinate (the same four roundings):
   no allowance of its own was needed.  Worst |err| / bound over the three families at (2, 45, 64), with and without dropout:
       act_feat 0.07   act_h 0.05 (fc1 / fc2 0.02)   act_c 0.15 (fc1 / fc2 0.09)   m 0.11   y 0.03   cos / cos freq / cos 15 pre 0.03 / 0.03 / 0.06
       act_go 0.69   act_g 0.32 (the head's 4-term product; below it 0.05)   g_pre / G freq / G phase 0.29 / 0.31 / 0.30   volume 0.02
   act_go's three roundings come close to their 3 u; a dot product of k terms stays near sqrt(k) / k of its bound, as it should.
2. Each corruption of the emulation's output that the kernels' hazards could produce exceeds a bound and is caught.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import field_backward_stage_common as S
from oracle import render_oracle as O

FAMILIES = {"film": "SHORTSIREN_FG", "res": "SHORTSIREN_FRes", "pfilm": "TALLSIREN"}
B, NPI, H = 2, 45, 64


def emulate(sn, case):
    """The stage in float32: (out dict of the chunk buffers and gradient volumes, saved rgb_sigma)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    nB, npi = case.points.shape[:2]
    n, Hh, L = nB * npi, sn.H, len(sn.kinds)
    pts = T(case.points)
    flat = pts.reshape(n, 3)
    cols = []
    for lvl, cc in S.input_tiles(sn, case.levels):
        if lvl < 0:
            cols.append(F.pad(flat, (0, 29)))
        elif cc == 0:
            vol = T(case.levels[lvl]).permute(0, 4, 1, 2, 3).contiguous()
            grid = (pts / (O.VOXEL_LENGTH / 2)).reshape(nB, 1, 1, npi, 3)
            f = F.grid_sample(vol, grid, mode="bilinear", align_corners=False, padding_mode="border")
            cols.append(f.reshape(nB, -1, npi).permute(0, 2, 1).reshape(n, -1))
    feat = torch.cat(cols, 1)
    rows = lambda t, i: T(t)[:, i * Hh:(i + 1) * Hh].repeat_interleave(npi, 0)

    def factor(d):
        if case.drop is None or d is None:
            return None
        p = torch.tensor(case.drop[0], dtype=torch.float32)
        return T(case.drop[1][d]).reshape(n, Hh).float() * (1.0 / (1.0 - p))

    def act(arg, d):
        f = factor(d)
        return (torch.sin(arg), torch.cos(arg)) if f is None else (torch.sin(arg) * f, torch.cos(arg) * f)

    W = lambda a: T(a)
    h, c = [], []
    if sn.pfilm:
        Wm1, bm1, Wm2, bm2 = (T(t) for t in sn.map)
        m = F.leaky_relu(F.linear(feat, Wm1, bm1), 0.2)
        fo = F.linear(m, Wm2, bm2)
        x = flat
        for l, mt in enumerate(sn.mats):
            pre = F.linear(x, W(mt.W), W(mt.b))
            f = fo[:, l * Hh:(l + 1) * Hh] * 15 + 30
            y, cs = act(f * pre + fo[:, (L + l) * Hh:(L + l + 1) * Hh], mt.drop)
            h.append(y)
            c += [cs, cs * f, cs * (15 * pre)]
            x = y
    else:
        k0 = sn.mats[0].W.shape[1]
        x = feat[:, :k0]
        for s, mt in enumerate(sn.mats):
            pre = F.linear(x, W(mt.W), W(mt.b))
            if mt.role == "fc2":
                pre = h[s - 2] + pre
            if mt.film is not None:
                pre = rows(case.freq, mt.film) * pre + rows(case.phase, mt.film)
            y, cs = act(pre, mt.drop)
            h.append(y)
            c.append(cs)
            x = y
    head = F.linear(x, T(sn.head_W), T(sn.head_b))
    saved = head.clone()
    if sn.sigmoid:
        saved[:, :3] = torch.sigmoid(head[:, :3])
    go = T(case.upstream).reshape(n, 4).clone()
    if sn.sigmoid:
        go[:, :3] = go[:, :3] * (saved[:, :3] * (1 - saved[:, :3]))
    gy = go @ T(sn.head_W)
    g = [None] * len(sn.mats)
    out = {}
    if sn.pfilm:
        Gf, Gp = [None] * L, [None] * L
        for l in range(L - 1, -1, -1):
            g[l], Gf[l], Gp[l] = gy * c[3 * l + 1], gy * c[3 * l + 2], gy * c[3 * l]
            gy = g[l] @ W(sn.mats[l].W)
        out["act_h"] = torch.cat([torch.stack(h).reshape(-1), m.reshape(-1)])
        out["act_g"] = torch.cat([torch.stack(g).reshape(-1), torch.cat(Gf + Gp, 1).reshape(-1)])
        out["grad_vols"] = []
    else:
        s = len(sn.mats) - 1
        while s >= 0:
            mt = sn.mats[s]
            if mt.role == "fc2":
                g[s] = gy * c[s]
                g[s - 1] = (g[s] @ W(mt.W)) * c[s - 1]
                gy = g[s - 1] @ W(sn.mats[s - 1].W) + g[s]
                s -= 2
                continue
            g[s] = gy * c[s]
            gpre = g[s] * rows(case.freq, mt.film) if mt.film is not None else g[s]
            if s:
                gy = gpre @ W(mt.W)
            s -= 1
        gvols = []
        W0 = T(sn.mats[0].W)
        img = torch.arange(nB).repeat_interleave(npi)
        for lvl, v in enumerate(case.levels):
            V, C = v.shape[1], v.shape[-1]
            gv = torch.zeros((nB * V ** 3, C))
            i0, lo, hi = O.trilinear_corners(pts, V)
            i0, lo, hi = i0.reshape(n, 3), lo.reshape(n, 3), hi.reshape(n, 3)
            for tk, (tl, cc) in enumerate(S.input_tiles(sn, case.levels)):
                if tl != lvl:
                    continue
                gfeat = gpre @ W0[:, 32 * tk:32 * tk + 32]
                for k in range(8):
                    d = torch.tensor([k & 1, (k >> 1) & 1, (k >> 2) & 1])
                    idx = torch.clamp(i0 + d, max=V - 1)
                    w = torch.where(d == 1, lo, hi).prod(1)
                    add = torch.zeros((n, C))
                    add[:, cc:cc + 32] = gfeat * w[:, None]
                    gv.index_add_(0, img * V ** 3 + (idx[:, 2] * V + idx[:, 1]) * V + idx[:, 0], add)
            gvols.append(gv.reshape(nB, V, V, V, C).numpy())
        out["act_h"], out["act_g"], out["grad_vols"] = torch.stack(h).reshape(-1), torch.stack(g).reshape(-1), gvols
    out["act_feat"], out["act_c"], out["act_go"] = feat.reshape(-1), torch.stack(c).reshape(-1), go.reshape(-1)
    for k in ("act_feat", "act_h", "act_c", "act_g", "act_go"):
        assert out[k].dtype == torch.float32
        out[k] = out[k].numpy().copy()
    return out, saved.reshape(nB, npi, 4).numpy()


def _honest(family, drop_p, seed=7):
    net, levels = S.make_net(FAMILIES[family], H, seed)
    sn = S.stage_net(net)
    case = S.random_case(net, levels, B, NPI, seed + 1, drop_p)
    with torch.no_grad():
        out, case.saved = emulate(sn, case)
    return sn, case, out


@pytest.fixture(scope="module")
def honest():
    """The emulation's output per family (without dropout), computed once and never modified: the corruptions work on copies."""
    return {family: _honest(family, 0.0) for family in FAMILIES}


@pytest.mark.parametrize("drop_p", [0.0, 0.3])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_honest_float32_emulation_stays_inside_every_bound(family, drop_p):
    sn, case, out = _honest(family, drop_p)
    S.check_forward_rows(sn, case, out)
    S.check_chain_rows(sn, case, out)


def _neighbour_row(sn, case, out):
    """one row of act_h taken from the neighbouring point"""
    h = out["act_h"].reshape(len(sn.mats), B * NPI, H)
    h[1, 17] = h[1, 18]


def _neighbour_freq(sn, case, out):
    """image 1 computed with image 0's freq"""
    wrong = copy.deepcopy(case)
    wrong.freq[1] = wrong.freq[0]
    out.update(emulate(sn, wrong)[0])


def _swapped_slabs(sn, case, out):
    """the two slabs of a residual block swapped"""
    s = next(i for i, m in enumerate(sn.mats) if m.role == "fc1")
    for k in ("act_h", "act_c", "act_g"):
        t = out[k].reshape(len(sn.mats), B * NPI, H)
        t[[s, s + 1]] = t[[s + 1, s]]


def _padded_lane_zero(sn, case, out):
    """a padded lane's zeros written over the last real row of an image in act_g (one 32-channel tile)"""
    out["act_g"].reshape(len(sn.mats), B * NPI, H)[2, NPI - 1, 32:64] = 0.0


def _missing_addend(sn, case, out):
    """one corner's addend missing from the gradient volume"""
    V = case.levels[0].shape[1]
    full = out["grad_vols"][0].copy()
    one = copy.deepcopy(case)
    one.upstream[0, 11] = 0.0                       # the volume without point 11 of image 0 ...
    without = emulate(sn, one)[0]["grad_vols"][0]
    (idx, w) = max(S.corner_list(case.points[0, 11:12], V), key=lambda iw: iw[1][0])
    v = np.unravel_index(int(idx[0]), (V, V, V))    # ... at that point's heaviest corner
    out["grad_vols"][0][0][v] = without[0][v]
    assert not np.array_equal(out["grad_vols"][0], full)


def _exchanged_halves(sn, case, out):
    """G's frequency and phase halves exchanged"""
    n, L = B * NPI, len(sn.kinds)
    G = out["act_g"][L * n * H:].reshape(n, 2 * L * H)
    G[:] = np.concatenate([G[:, L * H:], G[:, :L * H]], 1)


CORRUPTIONS = [("film", _neighbour_row, S.check_forward_rows), ("film", _neighbour_freq, S.check_forward_rows),
               ("res", _swapped_slabs, S.check_forward_rows), ("res", _swapped_slabs, S.check_chain_rows),
               ("film", _padded_lane_zero, S.check_chain_rows), ("res", _padded_lane_zero, S.check_chain_rows),
               ("film", _missing_addend, S.check_chain_rows), ("pfilm", _exchanged_halves, S.check_chain_rows)]


@pytest.mark.parametrize("family,corrupt,check", CORRUPTIONS, ids=[f"{f}-{c.__name__[1:]}-{k.__name__[6:]}" for f, c, k in CORRUPTIONS])
def test_corruption_exceeds_a_bound(honest, family, corrupt, check):
    sn, case, out = honest[family]
    bad = copy.deepcopy(out)
    with torch.no_grad():
        corrupt(sn, case, bad)
    with pytest.raises(AssertionError, match="act_|G |grad volume"):
        check(sn, case, bad)
