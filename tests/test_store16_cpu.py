"""What tests/test_gpu_store16.py holds the storing forward to, checked without a GPU (tests/store16_common.py):

1. An honest float32 emulation of the storing epilogue and both layouts passes every check of store16_common.check on every network of
   the GPU test -- so the reference arithmetic alone stays inside every condition -- and every case is usable: the reference's own fp32
   share beyond one fp16 ulp stays below 5 % at the last slab (measured: 0.0000 - 0.0038; the emulation's own 0.0000 - 0.0052; worst
   |err| / bound of the honest emulation: pair 0.50 - 0.70, sin 0.44 - 0.90, cos 0.44 - 0.91).
2. Each named hazard fails a check (measured on SHORTSIREN_FG / SHORTSIREN_FRes, H = 64, images 1..2 of 3, 350 points per image):
       cos quad halves swapped                  (b) pair identity 1023 x the bound (and (c) cos 4072 x)
       first pair from the previous quad        (c) sin 4054 x, cos 4069 x ((b) holds, 0.70: sine and cosine move together)
       sin and cos of neighbouring channels     (b) pair identity 1023 x (and (c) cos 4089 x)
       slab stride from the call's tiles        equalities: memory behind the chunk's tiles written, rows of the chunk left unwritten
       a padded lane that stores                equality: padded rows are the image's last point (the lane reads and stores the point of
                                                its own index instead: see store16_common's "rows past an image's end")
       an idle wave that stores                 equality: memory behind the chunk's tiles written; image 2's first tile fails (c), 3540 x
       freq of the wrong image                  (c) sin 4056 x on image 2's rows
       fc2 cosine without the identity          (b) pair identity 139 x (and (c) cos 138 x)
       leading fp16 part only in one matrix     the rgb_sigma equality, and (d): shares 0.27 / 0.48 / 0.70 in the slabs behind it against the
                                                reference's 0.0004 / 0.0010 / 0.0021; (c) does NOT see it (0.51): the hazard is the size of
                                                the stored operand's own rounding, which (c) must allow
       an un-clamped input tile at 7e4          equality: the tile is fp16(clamp(x)) (the hazard stores +inf)
3. cnerf_field_store16 refuses on the host, with CNERF_EINVAL and no launch (the addresses are made up), and is declared in the header
   and the ctypes prototypes."""
import ctypes
import os

import numpy as np
import pytest

import store16_common as K

NPI = K.R_RENDER * K.R_RENDER * K.S_RENDER


def _launch(cs, image0, n_images, npi, seed=11):
    return K.Launch(image0, n_images, K.random_points(cs, npi, seed)[image0:image0 + n_images])


@pytest.fixture(scope="module")
def hazard_cases():
    out = {}
    for variant in ("SHORTSIREN_FG", "SHORTSIREN_FRes"):
        cs, _ = K.make_case(variant, 64)
        la = _launch(cs, 1, 2, NPI)
        out[variant] = (cs, la, K.reference(cs, la))
    cs, _ = K.make_case("SHORTSIREN_FG", 64, hot_feature=7e4)
    out["hot"] = (cs, _launch(cs, 1, 2, NPI), None)
    return out


@pytest.mark.parametrize("variant,H", K.NETS)
def test_honest_emulation_passes_every_check(variant, H):
    cs, _ = K.make_case(variant, H)
    for image0, n_images, npi in ((1, 2, NPI), (2, 1, 33)):
        la = _launch(cs, image0, n_images, npi)
        em = K.emulate(cs, la)
        r = K.check(cs, la, dict(K.decode(cs, la, em), gather=em["gather"]), tag=f"{variant} H={H} npi={npi} ")
        assert not r.pop("broken")
        assert np.array_equal(em["rgb_sigma"], K.emulate(cs, la, storing=False)["rgb_sigma"])
        e2e = r.pop("e2e")
        print(f"{variant} H={H} npi={npi}: worst |err| / bound pair {max(v for k, v in r.items() if k.startswith('pair')):.3f}, "
              f"sin {max(v for k, v in r.items() if k.startswith('sin')):.3f}, cos {max(v for k, v in r.items() if k.startswith('cos')):.3f}; "
              f"last slab share {e2e[-1][0]:.4f} ({e2e[-1][1]:.1f} ulps), reference's fp32 {e2e[-1][2]:.4f} ({e2e[-1][3]:.1f} ulps)")


# hazard -> (case, what must happen: a ratio prefix that reaches 10, or the equality that breaks)
EXPECT = {
    "cos_quad_halves_swapped": ("SHORTSIREN_FG", "pair"),
    "first_pair_from_previous_quad": ("SHORTSIREN_FG", "sin"),
    "sincos_neighbour_channels": ("SHORTSIREN_FG", "pair"),
    "slab_stride_of_the_call": ("SHORTSIREN_FG", "memory behind the chunk's tiles was written"),
    "padded_lane_unclamped": ("SHORTSIREN_FG", "padded rows of h are not the image's last point"),
    "idle_wave_stores": ("SHORTSIREN_FG", "memory behind the chunk's tiles was written"),
    "freq_wrong_image": ("SHORTSIREN_FG", "sin"),
    "fc2_cos_without_identity": ("SHORTSIREN_FRes", "pair"),
    "leading_part_only": ("SHORTSIREN_FG", "rgb_sigma"),
    "input_unclamped": ("hot", "input tile 0 (level 0, channel 0) is not fp16(clamp(x))"),
}


@pytest.mark.parametrize("hazard", K.HAZARDS)
def test_hazard_fails_a_check(hazard_cases, hazard):
    name, expect = EXPECT[hazard]
    cs, la, ref = hazard_cases[name]
    with np.errstate(all="ignore"):
        bad = K.emulate(cs, la, hazard)
        r = K.check(cs, la, dict(K.decode(cs, la, bad), gather=bad["gather"]), ref=ref, strict=False, inputs_only=name == "hot")
    broken = r.pop("broken")
    e2e = r.pop("e2e", None)
    worst = {p: max([v for k, v in r.items() if k.startswith(p)], default=0.0) for p in ("pair", "sin", "cos")}
    print(f"{hazard}: worst |err| / bound {worst}; equalities broken: {sorted(set(broken))}" + (f"; (d) last slab {e2e[-1]}" if e2e else ""))
    if expect == "rgb_sigma":
        assert not np.array_equal(bad["rgb_sigma"], K.emulate(cs, la, storing=False)["rgb_sigma"])
        assert any("fp16 ulp of float64" in b for b in broken), "(d) sees single-pass products too"
        assert max(worst.values()) < 10.0, "(c) is not what catches it"
    elif expect in worst:
        assert worst[expect] >= 10.0, (hazard, worst)
    else:
        assert expect in broken, (hazard, broken)
    if hazard == "idle_wave_stores":
        assert worst["sin"] >= 10.0, "the next image's first tile holds the previous image's last point"
    if hazard == "slab_stride_of_the_call":
        assert "a row of the chunk was left unwritten (the canary is a NaN)" in broken
    if name != "hot" and expect != "rgb_sigma":
        with pytest.raises(AssertionError):
            K.check(cs, la, dict(K.decode(cs, la, bad), gather=bad["gather"]), ref=ref)


def test_layout_helpers_are_inverse_and_match_the_header_formula():
    NT, tiles, ns = 4, 3, 2
    rows = np.arange(ns * tiles * 32 * 32 * NT, dtype=np.float32).reshape(ns, tiles * 32, 32 * NT)
    assert np.array_equal(K.from_cos16(K.to_cos16(rows, NT), ns, tiles, NT), rows)
    assert np.array_equal(K.from_tb16(K.to_tb16(rows, NT), ns, tiles, NT), rows)
    tb, cs16 = K.to_tb16(rows, NT), K.to_cos16(rows, NT)
    for m, T, t, g, hh, e, j in ((1, 2, 3, 1, 1, 2, 17), (0, 0, 0, 0, 0, 0, 0), (1, 1, 2, 3, 0, 3, 31)):
        ch = 32 * t + 8 * g + 4 * hh + e
        assert cs16[((((m * tiles + T) * NT + t) * 4 + g) * 64 + j + 32 * hh) * 4 + e] == rows[m, T * 32 + j, ch]
        assert tb[(((m * tiles + T) * NT + t) * 32 + j) * 32 + ch % 32] == rows[m, T * 32 + j, ch]


def _cfg(L, kinds=(0, 0, 0, 0), B=3, R=5, S=7, V=5, C=32, flags=None, precision=None, drop_p=0.0):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, R, S, V, C, 64, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.voxel_length, cfg.fov_deg, cfg.ray_start, cfg.ray_end = 1.2, 30.0, 0.25, 1.95
    cfg.flags = L.F_SIGMOID_RGB | L.F_HIERARCHICAL if flags is None else flags
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
    assert "int cnerf_field_store16(" in header and "#define CNERF_ABI_VERSION 10" in header and lib.cnerf_abi_version() == 10
    assert lib.cnerf_field_store16.restype is ctypes.c_int and len(lib.cnerf_field_store16.argtypes) == 16
    one = ctypes.c_void_p(256)                                     # made up, aligned, never dereferenced: a refusal launches nothing
    vs = L.Volumes()
    vs.level[0] = 256
    A = dict(pss=0, i0=0, n=2, vols=ctypes.byref(vs), packed=one, freq=one, phase=one, cam=one, u=one, fz=one, feat=one, h=one, c=one, out=one)

    def call(cfg, **kw):
        a = dict(A, **kw)
        return lib.cnerf_field_store16(ctypes.byref(cfg), a["pss"], a["i0"], a["n"], a["vols"], a["packed"], a["freq"], a["phase"], a["cam"], a["u"],
                                       a["fz"], a["feat"], a["h"], a["c"], a["out"], None)

    err = lambda: lib.cnerf_last_error()
    cfg = _cfg(L)
    assert call(_cfg(L, kinds=(3, 3, 3))) == -22 and b"per-point FiLM" in err()
    assert call(_cfg(L, precision=L.PREC_FP32)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, precision=L.PREC_FP16)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, drop_p=0.1)) == -22 and b"drop" in err()
    assert call(_cfg(L, precision=L.PREC_FP32, drop_p=0.1)) == -22
    for pss in (-1, 3):
        assert call(cfg, pss=pss) == -22 and b"pass" in err()
    for i0, n in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2)):
        assert call(cfg, i0=i0, n=n) == -22 and b"image range" in err(), (i0, n)
    for k in ("vols", "packed", "feat", "h", "c", "out"):
        assert call(cfg, **{k: None}) == -22 and b"NULL" in err(), k
    assert call(cfg, vols=ctypes.byref(L.Volumes())) == -22 and b"volume level 0 is NULL" in err()
    assert call(cfg, freq=None) == -22 and b"freq" in err()
    assert call(cfg, phase=None) == -22 and b"phase" in err()
    assert call(cfg, cam=None) == -22 and b"cam2world" in err()
    assert call(cfg, pss=1, fz=None) == -22 and b"fine_z" in err()
    assert call(cfg, pss=2, u=None) == -22 and b"points" in err()
    assert call(_cfg(L, S=1)) == -22                                  # a cfg that describes no render
