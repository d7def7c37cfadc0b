"""What tests/test_gpu_store_pw16.py holds the per-point FiLM storing forward to, checked without a GPU (tests/store_pw16_common.py):

1. An honest float32 emulation of field_pw16_kernel<STORE>'s and pw_deriv_kernel's arithmetic passes every check on every network of the
   GPU test (350, 33 and 128 points per image), and every case is usable: |A| <= 300 (measured: 25 - 40 on the default nets, 50 - 73 on
   the range nets, 0.7 on the quiet one), the reference's own fp32 share beyond one fp16 ulp below 5 % at the last layer of every network
   (d) applies to (0.0000 - 0.0021), and every |cos f|, |cos 15 pre| of the quiet net below 0.9 in float64 (0.51; its amax are all 1.0).
   Worst |err| / bound of the honest emulation: pair 0.53 - 0.70, m 0.94 - 0.98 (one fp16 rounding, attained), sin / cos 0.51 - 0.85,
   cos f 0.01 - 0.82, cos 15 pre 0.87 - 0.98 (one fp16 rounding again), amax up to 1.00 of its rounding allowance.  pw_deriv's f and
   15 pre BEFORE the cosine and the store against float64 from the same stored operands, per element with |value| >= 1, default nets:
   f 4.5e-5 - 1.1e-4 (the kernel's comment: 1e-4), 15 pre 0.8e-3 - 2.8e-3, at elements whose sum cancels (1.2e-4 - 2.1e-4 of the row's
   largest value).  The kernel's comment used to claim "relative 6e-4" for 15 pre; it now says what is measured.  Both rows are held
   to the bound of (e), which carries h sum |W| |x| and so allows for the cancellation.
2. Each named hazard fails the named condition (default net, H = 64, images 1..2 of 3, 350 points per image; the floor on the quiet net):
       cos from its own reduction (no phase term)      (b) pair identity 614 x (and (c) cos 4080 x)
       f without the + 30                              (e) cos f 1806 x
       operand's low part dropped in fr / ph           (c) sin 2.8 x, cos 2.7 x from layer 0 on -- built on the fp32 feature; (d) sees it too
       derivative rows of the previous output tile     (e) cos f, cos 15 pre
       phase rows at (l + 1) H                         (c) sin 7324 x
       pw_deriv reads y_l for layer l's pre            (e) cos 15 pre 1912 x, layers 1..7
       pw_deriv's weight pieces one KiB off (low)      (e) cos f 447 x, cos 15 pre 2031 x
       weight unit one slot stale, second trip         (c) sin 5691 x on the rows of every block's second group
       amax from one lane half                         amax: a stored derivative exceeds amax (1 + h)
       amax without its floor                          amax is not exactly 1 (quiet net)
       m stored before the LeakyReLU                   (c) m 8115 x
       padded rows left unwritten                      (a) finite; padded rows are the image's last point
       position tile columns 3..31 not zero            (a)
       position rounded toward zero                    (a) the position tile
       cos slabs at stride 1                           (a) finite (slab 3 l never written for most l); (b), (c) cos
3. cnerf_field_store_pw16 refuses on the host, with CNERF_EINVAL and no launch, and include/cnerf.h declares what _lib.py binds."""
import ctypes
import os

import numpy as np
import pytest

import store_pw16_common as K

NPI = K.R_RENDER * K.R_RENDER * K.S_RENDER
RATIOS = ("pair", "m", "sin", "cos", "cosf", "cosp", "amax")


def _launch(cs, image0, n_images, npi, seed=11):
    pts = K.random_points(cs, npi, seed)
    if cs.kind == "hot":
        pts[1, 0] = K.HOT_CENTRE
    return K.Launch(image0, n_images, pts[image0:image0 + n_images])


def _judge(cs, la, em, ref, strict=True):
    return K.check(cs, la, dict(K.decode(cs, la, em), gather=em["gather"]), ref=ref, strict=strict, tag=f"{cs.name} npi={la.npi} ")


@pytest.mark.parametrize("name", list(K.NETS))
def test_honest_emulation_passes_every_check(name):
    cs, _ = K.make_case(name)
    for image0, n_images, npi in ((1, 2, NPI), (2, 1, 33), (0, 3, 128)):
        la = _launch(cs, image0, n_images, npi)
        ref = K.reference(cs, la)
        em = K.emulate(cs, la)
        r = _judge(cs, la, em, ref)
        assert not r.pop("broken")
        print(f"{name} npi={npi}: {K.summary(r)}; pw_deriv's f / 15 pre before the cosine: {em['f_rel']:.2e} / {em['p_rel']:.2e}")
        assert ref[2] <= 300.0, "the case leaves VSIN's range"
        if cs.e2e:
            assert ref[1][-1][0] < 0.05, "the reference's own fp32 evaluation is too far from float64 for (d)"
        else:
            assert not r["e2e"]
        if cs.kind == "quiet":
            assert ref[3] < 0.9, "the quiet net is not quiet"
            assert (K.decode(cs, la, em)["amax"] == 1.0).all()
        if cs.kind == "hot" and image0 <= 1 < image0 + n_images:
            hot = K.hot_rows(cs, la)
            assert hot.any() and (np.abs(em["gather"][hot]) > 65504.0).any(), "no point reads the hot voxel beyond fp16's range"
            feat = K.decode(cs, la, em)["feat"][la.valid][hot]
            assert (np.abs(feat[:, :32]).max() == 65504.0) and np.isfinite(feat).all()
        # two emulations of the same inputs: the same bits (the GPU test's repeatability condition has something to compare)
        again = K.emulate(cs, la)
        assert all(np.array_equal(em[k], again[k], equal_nan=True) for k in ("feat", "h", "c", "amax", "rgb_sigma"))


# hazard -> (case, a ratio that must exceed 1, or the words of the equality that breaks)
EXPECT = {
    "cos_own_reduction": ("default64", "pair"),
    "f_without_30": ("default64", "cosf"),
    "operand_low_part_dropped": ("default64", "sin"),
    "deriv_rows_of_previous_tile": ("default64", "cosf"),
    "phase_rows_at_next_layer": ("default64", "sin"),
    "deriv_pre_from_y_l": ("default64", "cosp"),
    "deriv_low_pieces": ("default64", "cosf"),
    "stale_unit_second_trip": ("default64", "sin"),
    "amax_one_lane_half": ("default64", "a stored derivative exceeds amax (1 + h)"),
    "amax_without_floor": ("quiet", "is not exactly 1 where every stored derivative is below 1"),
    "m_before_leaky": ("default64", "m"),
    "padded_rows_unwritten": ("default64", "padded rows of y are not the image's last point"),
    "position_tile_tail": ("default64", "columns 3..31 of the position tile are not zero"),
    "position_truncated": ("default64", "the position tile is not fp16 (nearest even) of the positions"),
    "cos_slab_stride_1": ("default64", "an element of the chunk's tiles is not finite (the canary is a NaN)"),
}


@pytest.fixture(scope="module")
def hazard_cases():
    out = {}
    for name in ("default64", "quiet"):
        cs, _ = K.make_case(name)
        la = _launch(cs, 1, 2, NPI)
        out[name] = (cs, la, K.reference(cs, la))
    return out


@pytest.mark.parametrize("hazard", K.HAZARDS)
def test_hazard_fails_a_check(hazard_cases, hazard):
    name, expect = EXPECT[hazard]
    cs, la, ref = hazard_cases[name]
    with np.errstate(all="ignore"):
        bad = K.emulate(cs, la, hazard)
        r = _judge(cs, la, bad, ref, strict=False)
    broken = r.pop("broken")
    print(f"{hazard}: worst |err| / bound " + " ".join(f"{k} {r[k]:.3g}" for k in RATIOS) + f"; broken: {sorted(set(b.split(' is ')[0] for b in broken))[:6]}")
    if expect in RATIOS:
        assert r[expect] > 1.0, (hazard, r)
        if hazard != "operand_low_part_dropped":       # (the size of the low part itself: 2^-11 of the operand against a bound of 2^-19 + roundings)
            assert r[expect] >= 10.0, (hazard, r)
    else:
        assert any(expect in b for b in broken), (hazard, broken)
    if hazard == "operand_low_part_dropped":
        assert r["m"] <= 1.0 and r["cosf"] <= 1.0 and r["cosp"] <= 1.0, "only (c) and (d) can see it: what pw_deriv reads is stored"
    if hazard == "stale_unit_second_trip":
        honest = _judge(cs, la, K.emulate(cs, la), ref)
        assert honest["sin"] <= 1.0
    with pytest.raises(AssertionError):
        _judge(cs, la, bad, ref)


def test_long_shape_gives_every_block_two_or_three_groups():
    for cus in (256, 304, 120, 64):
        R, S_ = K.long_shape(cus)
        npi = R * R * S_
        groups = 2 * (((npi + 31) // 32 + 3) // 4)
        assert 2 <= S_ <= 128 and npi % 32 and groups % 8 and 2.3 * cus <= groups <= 2.7 * cus, (cus, R, S_, groups)


def _cfg(L, kinds=(3, 3, 3), B=3, R=5, S=7, V=5, C=32, precision=None, drop_p=0.0):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, R, S, V, C, 64, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.voxel_length, cfg.fov_deg, cfg.ray_start, cfg.ray_end = 1.2, 30.0, 0.25, 1.95
    cfg.flags = L.F_HIERARCHICAL
    cfg.precision = L.PREC_FP16X3 if precision is None else precision
    cfg.drop_p = drop_p
    return cfg


def test_entry_refuses_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(ge.__file__)), "include", "cnerf.h")).read()
    assert "int cnerf_field_store_pw16(" in header and "#define CNERF_ABI_VERSION 10" in header and lib.cnerf_abi_version() == 10
    assert lib.cnerf_field_store_pw16.restype is ctypes.c_int and len(lib.cnerf_field_store_pw16.argtypes) == 15
    decl = header[header.index("int cnerf_field_store_pw16("):]
    assert decl[:decl.index(";")].count(",") == 14, "the header's argument list is what _lib.py binds"
    assert L.LAYER_PFILM == 3
    one = ctypes.c_void_p(256)                                     # made up, aligned, never dereferenced: a refusal launches nothing
    vs = L.Volumes()
    vs.level[0] = 256
    A = dict(pss=0, i0=0, n=2, vols=ctypes.byref(vs), packed=one, cam=one, u=one, fz=one, feat=one, h=one, c=one, amax=one, out=one)

    def call(cfg, **kw):
        a = dict(A, **kw)
        return lib.cnerf_field_store_pw16(ctypes.byref(cfg), a["pss"], a["i0"], a["n"], a["vols"], a["packed"], a["cam"], a["u"], a["fz"], a["feat"], a["h"],
                                          a["c"], a["amax"], a["out"], None)

    err = lambda: lib.cnerf_last_error()
    cfg = _cfg(L)
    assert call(_cfg(L, kinds=(0, 0, 0, 0))) == -22 and b"per-point FiLM networks only" in err()
    assert call(_cfg(L, precision=L.PREC_FP32)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, precision=L.PREC_FP16)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, drop_p=0.1)) == -22 and b"drop" in err()
    assert call(_cfg(L, C=64)) == -22 and b"32-channel" in err()
    two = _cfg(L, C=64)
    two.n_levels, two.level_V[0], two.level_V[1], two.level_C[0], two.level_C[1] = 2, 5, 3, 32, 32
    assert call(two) == -22 and b"32-channel" in err()
    for pss in (-1, 3):
        assert call(cfg, pss=pss) == -22 and b"pass" in err()
    for i0, n in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert call(cfg, i0=i0, n=n) == -22 and b"image range" in err(), (i0, n)
    for k in ("vols", "packed", "feat", "h", "c", "amax", "out"):
        assert call(cfg, **{k: None}) == -22 and b"NULL" in err(), k
    assert call(cfg, vols=ctypes.byref(L.Volumes())) == -22 and b"volume level 0 is NULL" in err()
    assert call(cfg, cam=None) == -22 and b"cam2world" in err()
    assert call(cfg, pss=1, fz=None) == -22 and b"fine_z" in err()
    assert call(cfg, pss=2, u=None) == -22 and b"points" in err()
    assert call(_cfg(L, S=1)) == -22                                  # a cfg that describes no render
