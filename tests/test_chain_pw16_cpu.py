"""What tests/test_gpu_chain_pw16.py holds chain_pre_kernel and pw_gm_kernel to, checked without a GPU (tests/chain_pw16_common.py):

1. The dry runs' sampling rule (groups / 1024, clamped to 1..32) on top of the sampled-groups restatement of tests/chain16_common.py,
   which tests/test_chain16_cpu.py holds against group_range()'s documented rule, and the populations the cases rely on: idle waves and
   ragged last tiles, NT = 2 / 4 / 8, 8 / 2 / 1 layers, three passes, an image sub-range, the hot points in an unsampled group, padded
   rows with values of their own.
2. An honest float32 NumPy emulation of the two kernels' arithmetic stays inside every bound and meets every equality on every case of
   the GPU test: the bounds are attainable.
3. Each named hazard, applied to the emulation, exceeds a bound by at least 10 x on the case named for it, or breaks the equality named
   for it (the table HAZARD_CASE; each run prints by what).  "operand_range_unreported" is chain_pre_kernel as it was before it reported
   the range of pw_gm's operands gy16 d To: on the intermediate case every g_mpre of the hot point is a NaN while `saturated` stays 0.
4. cnerf_field_chain_pw16 refuses on the host, with CNERF_EINVAL and no launch (the addresses are made up)."""
import ctypes
import os

import numpy as np
import pytest

import chain_pw16_common as K


@pytest.fixture(scope="module")
def cases():
    """name -> (case, honest emulation's outputs): computed once, never modified."""
    out = {}
    for name in K.CASES:
        cs = K.case(name)[0]
        out[name] = (cs, K.emulate(cs))
    return out


def test_sampling_rule_and_the_populations_of_the_cases(cases):
    assert K.production_step(2, 32) == 1 and K.production_step(1, 4 * 2048) == 2 and K.production_step(1, 4 * 2047) == 1
    assert K.production_step(64, 4096 * 64) == 32 and K.production_step(8, 4 * 8192) == 32 and K.production_step(1, 4 * 31 * 1024) == 31
    assert K.sampled_groups(2, 32, 2) == list(range(0, 16, 2))
    for name, (cs, _) in cases.items():
        if cs.npi == 175:          # 6 tiles: two idle waves per image, a 15-row last tile
            assert cs.tpi == 6 and K.idle_waves(cs.n_images, cs.tpi) == 2 * cs.n_images and cs.npi - 32 * 5 == 15
        elif cs.npi == 33:         # 2 tiles: two idle waves per image, a 1-row last tile
            assert cs.tpi == 2 and K.idle_waves(cs.n_images, cs.tpi) == 2 * cs.n_images
        else:
            assert "step" in name and cs.npi == 1024 and cs.tpi == 32 and K.idle_waves(2, 32) == 0
        pad = ~cs.valid
        assert pad.any() or cs.npi == 1024
        if pad.any():              # padded rows: values of their own, the extremes among them; amax's move r_l in the even layers
            assert (np.abs(cs.cos[:, pad].astype(np.float64)) == 65504).all() and (np.abs(cs.m16[pad].astype(np.float64)) == 65504).all()
            for l in range(cs.L):
                real, every = cs.amax[l][cs.valid].max(), cs.amax[l].max()
                assert (every > real and K.r_of(every) < K.r_of(real)) if l % 2 == 0 else every == real, (name, l)
        # the derivative rows: realistic magnitudes, exact 0 and +-1; amax is the float32 maximum of the supplied rows; m16 has both signs and zeros
        c = cs.cos[:, cs.valid].astype(np.float64)
        assert (c == 1).any() and (c == -1).any() and (c == 0).any()
        assert np.abs(c[0::3]).max() <= 1 and 30 < np.abs(c[1::3]).max() <= 40 and 15 < np.abs(c[2::3]).max() <= 32
        for l in range(cs.L):
            assert np.array_equal(cs.amax[l][cs.valid], np.abs(cs.cos[3 * l:3 * l + 3][:, cs.valid].astype(np.float32)).max(axis=(0, 2)))
        m = cs.m16[cs.valid].astype(np.float64)
        assert (m > 0).any() and (m < 0).any() and (m == 0).any()
    assert {c[0].sn.H for c in cases.values()} == {64, 128, 256} and {c[0].pss for c in cases.values()} == {0, 1, 2}
    assert {c[0].L for c in cases.values()} == {1, 2, 8} and any(c[0].image0 == 1 and c[0].B == 3 for c in cases.values())
    assert any(np.abs(c[0].base).max() > 0 for c in cases.values())
    cs = cases["sampling_step2"][0]
    sampled = K.tiles_of_groups(K.sampled_groups(2, 32, 2), 32)
    assert len(sampled) == 32 and cs.hot[0] == 1 and (32 + cs.hot[1] // 32) not in sampled
    big = np.abs(cs.upstream[1, cs.hot[1]]).max()
    rest = np.delete(np.abs(cs.upstream).reshape(-1, 4), 1024 + cs.hot[1], axis=0).max()
    assert big == np.float32(2.0 ** 20) * rest
    assert np.array_equal(cases["sampling_step1"][0].upstream, cs.upstream) and cases["sampling_step1"][0].hot is None
    # the intermediate case: the hot point's last-layer g_y is stored unclamped, 15.9 x the sampled binade, and its operands leave fp16's range
    cs, out = cases["intermediate_step2"]
    hot_row = cs.hot[0] * cs.tpi * 32 + cs.hot[1]
    assert (32 + cs.hot[1] // 32) not in sampled
    top = np.abs(out["gy"][cs.L - 1][hot_row]).max()
    assert 32000 < top < 65504 / 2 and not out["gy"][:cs.L - 1, hot_row].any()
    rest = np.delete(np.abs(out["gy"][cs.L - 1]).max(axis=1), hot_row).max()
    assert 1024 < rest <= 2048
    up = np.abs(cases["wide128_coarse"][0].upstream[0, :21]).max(axis=1)
    assert up[0] / up[20] > 2.0 ** 17
    sy = cases["wide128_coarse"][1]["scales"][2 * (3 * 8 + 2)::2][:8]
    assert np.abs(np.diff(np.log2(sy))).min() >= 4, "consecutive layers' g_y scales several binades apart"
    cs = cases["copies64_fine"][0]
    assert np.array_equal(cs.upstream[:, 18], cs.upstream[:, 0] * np.float32(2.0 ** -18)) and np.array_equal(cs.cos[:, 18], cs.cos[:, 0])


def _sat_of(cs):
    return {"sampling_step2": cs.L, "intermediate_step2": 1}.get(cs.name, 0)


@pytest.mark.parametrize("name", list(K.CASES))
def test_honest_float32_emulation_stays_inside_the_bound(cases, name):
    cs, out = cases[name]
    r = K.check(cs, out, name + " ")
    assert not r.pop("broken")
    print(f"{name}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; saturated {out['sat']}")
    assert out["sat"] == _sat_of(cs)       # the hot tile in each layer; the intermediate hot tile in the last layer alone (no g_y below)
    if name in K.WHOLE_CHAIN:
        assert K.whole_chain_rel_l2(cs, out["vols"]) <= 2e-3


#            hazard                    the case named for it, what must happen there (None: a bound exceeded 10 x)
HAZARD_CASE = {
    "cosf_from_cos15":       ("pw64_coarse", None),
    "row_slot_stale":        ("pw64_image_range", "the stored slabs are fp16(gy16 d16 r_l) bit for bit"),
    "gy_prev_layer":         ("pw128_fine", "the stored slabs are fp16(gy16 d16 r_l) bit for bit"),
    "fr_ph_swapped":         ("pw256_points", None),
    "rho_skipped":           ("wide128_coarse", None),
    "rho_seven_of_eight":    ("wide64_points", None),
    "stale_weight_unit":     ("shallow2_64_points", None),
    "slope_neighbour_tile":  ("shallow1_64_fine", None),
    "Tm_half_row":           ("pw128_points_tail1", None),
    "T_per_tile":            ("copies64_fine", "g_y rows of power-of-two copies are exact multiples"),
    "padded_lane_stores":    ("pw128_fine", "rows past an image's end are zero"),
    "padded_lane_scatters":  ("pw64_coarse", None),
    "gmax_wrong_slot":       ("wide128_coarse", "g_y scale"),
    "operand_range_unreported": ("intermediate_step2", "the contract: outputs finite and in bound, or saturated > 0"),
}


@pytest.mark.parametrize("hazard", K.HAZARDS)
def test_hazard_exceeds_the_bound_or_breaks_its_equality(cases, hazard):
    name, equality = HAZARD_CASE[hazard]
    cs, honest = cases[name]
    bad = K.emulate(cs, hazard)
    assert bad["sat"] != honest["sat"] or not all(np.array_equal(bad[k], honest[k], equal_nan=True) for k in ("go16", "gy", "g", "gmp", "scales", "vols"))
    with np.errstate(all="ignore"):
        r = K.check(cs, bad, strict=False)
    broken = r.pop("broken")
    worst = max(r.values())
    print(f"{hazard}: worst |err| / bound {worst:.3g} on {name}; equalities broken: {sorted(set(broken))}")
    if equality is None:
        assert worst >= 10.0, (hazard, name, r)
    else:
        assert equality in broken, (hazard, name, broken)
    with pytest.raises(AssertionError), np.errstate(all="ignore"):
        K.check(cs, bad, name + " ")


def test_unreported_operand_range_gives_nan_with_saturated_zero(cases):
    """chain_pre_kernel before it reported the range of pw_gm's operands, on the intermediate case: the hot point's g_y is stored finite (chain_pre counts
    nothing), its operands gy16 d To are +-inf in about half the channels with both signs, every g_mpre of the point is a NaN, fmaxf
    drops them all, and `saturated` stays 0 while NaN goes into the volume: the documented contract did not hold."""
    cs, _ = cases["intermediate_step2"]
    bad = K.emulate(cs, "operand_range_unreported")
    hot_row = cs.hot[0] * cs.tpi * 32 + cs.hot[1]
    assert bad["sat"] == 0 and np.isnan(bad["gmp"][hot_row]).all() and np.isnan(bad["vols"]).any()
    assert np.isfinite(np.delete(bad["gmp"], hot_row, axis=0)).all()
    now = cases["intermediate_step2"][1]      # the same NaN today, reported: saturated = 1
    assert now["sat"] == 1 and np.isnan(now["gmp"][hot_row]).all()


def _cfg(L, kinds=(3, 3), B=2, R=5, S=7, V=5, C=32, precision=None):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, R, S, V, C, 64, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.voxel_length, cfg.fov_deg, cfg.ray_start, cfg.ray_end = 1.2, 30.0, 0.25, 1.95
    cfg.flags = L.F_HIERARCHICAL
    cfg.precision = L.PREC_FP16X3 if precision is None else precision
    return cfg


def test_entry_refuses_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(ge.__file__)), "include", "cnerf.h")).read()
    assert "int cnerf_field_chain_pw16(" in header and "#define CNERF_ABI_VERSION 10" in header and lib.cnerf_abi_version() == 10
    assert L.LAYER_CODE["pfilm"] == 3
    one = ctypes.c_void_p(256)                                     # made up, aligned, never dereferenced: a refusal launches nothing
    gv = L.Volumes()
    gv.level[0] = 256
    A = dict(pss=0, i0=0, n=2, packed=one, cam=one, u=one, fz=one, up=one, saved=one, cos=one, amax=one, m16=one, step=0, gy16=one, g16=one, go16=one,
             scales=one, gmax=one, gvols=ctypes.byref(gv), sat=None)

    def call(cfg, **kw):
        a = dict(A, **kw)
        return lib.cnerf_field_chain_pw16(ctypes.byref(cfg), a["pss"], a["i0"], a["n"], a["packed"], a["cam"], a["u"], a["fz"], a["up"], a["saved"], a["cos"],
                                          a["amax"], a["m16"], a["step"], a["gy16"], a["g16"], a["go16"], a["scales"], a["gmax"], a["gvols"], a["sat"], None)

    err = lambda: lib.cnerf_last_error()
    cfg = _cfg(L)
    assert call(_cfg(L, kinds=(0, 0, 0, 0))) == -22 and b"per-point FiLM networks only" in err()
    assert call(_cfg(L, precision=L.PREC_FP32)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, precision=L.PREC_FP16)) == -22 and b"FP16X3" in err()
    for pss in (-1, 3):
        assert call(cfg, pss=pss) == -22 and b"pass" in err()
    for i0, n in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
        assert call(cfg, i0=i0, n=n) == -22 and b"image range" in err(), (i0, n)
    assert call(cfg, step=-1) == -22 and b"group_step" in err()
    for k in ("packed", "up", "saved", "cos", "amax", "m16", "gy16", "g16", "go16", "scales", "gmax", "gvols"):
        assert call(cfg, **{k: None}) == -22 and b"NULL" in err(), k
    assert call(cfg, cam=None) == -22 and b"cam2world" in err()
    assert call(cfg, pss=1, fz=None) == -22 and b"fine_z" in err()
    assert call(cfg, pss=2, u=None) == -22 and b"points" in err()
    assert call(cfg, gvols=ctypes.byref(L.Volumes())) == -22 and b"gradient volume 0 is NULL" in err()
    assert call(_cfg(L, S=1)) == -22                                  # a cfg that describes no render
