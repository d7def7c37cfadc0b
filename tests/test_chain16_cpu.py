"""What tests/test_gpu_chain16.py holds chain16_kernel to, checked without a GPU (tests/chain16_common.py):

1. The restatement of the dry run's sampled tile groups, and the populations the cases rely on: idle waves and a ragged last tile in the
   175- and 33-point shapes, two groups per class in the sampling case, the hot point in an unsampled group of image 1.
2. An honest float32 NumPy emulation of the kernel's arithmetic -- fp16 conversions at the two conversion points, per-point T, per-slab S
   from the sampled maxima, the clamp -- stays inside the bound on every case of the GPU test, and satisfies every equality: the bound is
   attainable.  Worst |err| / bound: go16 0.99, the head's slab 0.76 - 0.89, lower slabs 0.09 - 0.34 (0.84 - 0.99 where the rows' floor
   FL / S is the whole bound: the wide-range and copies cases, image 1 of the 2^6 frequencies, the sampling case once the hot point sets
   the scales), gin 0.05 - 0.24, volumes 0.09 - 0.18.
3. Each named hazard, applied to the emulation, exceeds the bound by at least 10 x on the case named for it, or breaks the equality
   named for it.  The operand scale per tile is caught by the exact covariance of the "copies" cases: at a span of 2^24 it stays at
   2.6 x the row bound of the wide-range case (chain16_common's docstring says why).
4. cnerf_field_chain16 refuses on the host, with CNERF_EINVAL and no launch (the addresses are made up)."""
import ctypes
import os

import numpy as np
import pytest

import chain16_common as K


@pytest.fixture(scope="module")
def cases():
    """name -> (case, honest emulation's outputs): computed once, never modified."""
    out = {}
    for name in K.CASES:
        cs = K.case(name)[0]
        out[name] = (cs, K.emulate(cs))
    return out


def test_sampled_groups_and_the_populations_of_the_cases(cases):
    # every step-th group from each class's first; the number of blocks does not enter
    assert K.sampled_groups(2, 32, 1) == list(range(16))
    assert K.sampled_groups(2, 32, 2) == list(range(0, 16, 2))                   # two groups per class: the first of each
    assert K.sampled_groups(2, 6, 1) == [0, 1, 2, 3]                               # 4 groups: classes 1, 3, 5, 7 own one each
    assert K.sampled_groups(1, 80, 3) == [0, 2, 5, 7, 10, 12, 15, 17]              # 20 groups: 2 | 3 | 2 | 3 ..., first of each class
    assert K.sampled_groups(3, 45, 5) == [0, 4, 9, 13, 18, 22, 27, 31]             # 36 groups: 4 | 5 | 4 | 5 ...
    assert K.production_step(2, 32) == 1 and K.production_step(1, 4 * 4096) == 2 and K.production_step(1, 4 * 4095) == 1 and K.production_step(64, 4096 * 64) == 16
    # the restatement against a brute-force walk of the blocks, for several grid sizes
    for n_images, tpi, step in ((2, 32, 2), (3, 45, 5), (1, 80, 3), (2, 6, 1)):
        total = n_images * ((tpi + 3) // 4)
        for nblk in (8, 16, 24, 256):
            seen = []
            for blk in range(nblk):
                cls, idx, per = blk & 7, blk >> 3, (nblk + 7 - (blk & 7)) // 8
                seen += list(range(total * cls // 8 + idx * step, total * (cls + 1) // 8, per * step))
            assert sorted(seen) == K.sampled_groups(n_images, tpi, step), (n_images, tpi, step, nblk)
    assert K.tiles_of_groups([0, 1, 2, 3], 6) == list(range(12))                   # 2 images x 6 tiles: the idle waves own none
    for name, (cs, _) in cases.items():
        if cs.npi == 175:          # 6 tiles: two idle waves per image, a 15-row last tile
            assert cs.tpi == 6 and K.idle_waves(cs.n_images, cs.tpi) == 2 * cs.n_images and cs.npi - 32 * 5 == 15
        elif cs.npi == 33:         # 2 tiles: two idle waves per image, a 1-row last tile
            assert cs.tpi == 2 and K.idle_waves(cs.n_images, cs.tpi) == 2 * cs.n_images
        else:
            assert name.startswith("sampling") and cs.npi == 1024 and cs.tpi == 32 and K.idle_waves(2, 32) == 0
        assert (~cs.valid).any() or cs.npi == 1024
    cs = cases["sampling_step2"][0]
    sampled = K.tiles_of_groups(K.sampled_groups(2, 32, 2), 32)
    assert len(sampled) == 32 and cs.hot[0] == 1 and (32 + cs.hot[1] // 32) not in sampled
    big = np.abs(cs.upstream[1, cs.hot[1]]).max()
    rest = np.delete(np.abs(cs.upstream).reshape(-1, 4), 1024 + cs.hot[1], axis=0).max()
    assert big == np.float32(2.0 ** 20) * rest
    assert np.array_equal(cases["sampling_step1"][0].upstream, cs.upstream) and cases["sampling_step1"][0].hot is None
    assert {c[0].sn.H for c in cases.values()} == {64, 128, 256} and {c[0].pss for c in cases.values()} == {0, 1, 2}
    assert any(c[0].image0 == 1 for c in cases.values())
    # exact +-1 and 0 among the cosines, the wide range, the copies
    for cs, _ in cases.values():
        c = cs.cos.astype(np.float64)
        assert (c == 1).any() and (c == -1).any() and (c == 0).any() and np.abs(c).max() <= 1
    up = np.abs(cases["wide128_coarse"][0].upstream[0, :25]).max(axis=1)
    assert up[0] / up[24] > 2.0 ** 20
    cs = cases["copies_dgx128"][0]
    assert np.array_equal(cs.upstream[:, 24], cs.upstream[:, 0] * np.float32(2.0 ** -24)) and np.array_equal(cs.cos[:, 24], cs.cos[:, 0])
    f = cases["fg128_freq64"][0].freq
    assert np.array_equal(f[1], f[0] * np.float32(2.0 ** -6))


@pytest.mark.parametrize("name", list(K.CASES))
def test_honest_float32_emulation_stays_inside_the_bound(cases, name):
    cs, out = cases[name]
    r = K.check(cs, out, name + " ")
    assert not r["broken"]
    assert out["sat"] == (4 if name == "sampling_step2" else 0)       # the hot point's tile in each of the four slabs


#            hazard                 the case named for it, what must happen there
HAZARD_CASE = {
    "cos_quad_half":      ("fg256_points", None),
    "film_prev_slab":     ("fg64_coarse", None),
    "film_image0":        ("fg64_image_range", None),
    "identity_dropped":   ("res256_coarse", None),
    "identity_prev_T":    ("res2_128_points", None),
    "scale_per_tile":     ("copies_dres64", "gin rows of power-of-two copies are exact multiples"),
    "stale_weight_unit":  ("sine256_coarse", None),
    "padded_lane_stores": ("dgx64_fine", "rows past an image's end are zero"),
    "gmax_slab_shift":    ("pyrmd128_coarse", "slab scale"),
}


@pytest.mark.parametrize("hazard", K.HAZARDS)
def test_hazard_exceeds_the_bound_or_breaks_its_equality(cases, hazard):
    name, equality = HAZARD_CASE[hazard]
    cs, honest = cases[name]
    with np.errstate(all="ignore"):
        bad = K.emulate(cs, hazard)
    assert not all(np.array_equal(bad[k], honest[k]) for k in ("go16", "g", "scales"))
    r = K.check(cs, bad, strict=False)
    broken = r.pop("broken")
    worst = max(r.values())
    print(f"{hazard}: worst |err| / bound {worst:.3g} on {name}; equalities broken: {sorted(set(broken))}")
    if equality is None:
        assert worst >= 10.0, (hazard, name, r)
    else:
        assert equality in broken, (hazard, name, broken)
    with pytest.raises(AssertionError):
        K.check(cs, bad, name + " ")


def test_per_tile_scale_on_the_wide_range_case_is_measured(cases):
    """The span of 2^24 the wide-range case has leaves a per-tile operand scale within a small multiple of the row bound (the stored
    rows' floor is as coarse): the figure is printed, the hazard is carried by the copies' equality above."""
    cs, _ = cases["wide128_coarse"]
    r = K.check(cs, K.emulate(cs, "scale_per_tile"), strict=False)
    print("scale_per_tile on wide128_coarse: worst |err| / bound", max(v for k, v in r.items() if k != "broken"))
    assert max(v for k, v in r.items() if k != "broken") > 1.0


def _cfg(L, kinds=(0, 0, 0, 0), B=2, R=5, S=7, V=5, C=32, flags=None, precision=None):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, R, S, V, C, 64, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.voxel_length, cfg.fov_deg, cfg.ray_start, cfg.ray_end = 1.2, 30.0, 0.25, 1.95
    cfg.flags = L.F_SIGMOID_RGB | L.F_HIERARCHICAL if flags is None else flags
    cfg.precision = L.PREC_FP16X3 if precision is None else precision
    return cfg


def test_entry_refuses_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(ge.__file__)), "include", "cnerf.h")).read()
    assert "int cnerf_field_chain16(" in header and "#define CNERF_ABI_VERSION 10" in header and lib.cnerf_abi_version() == 10
    one = ctypes.c_void_p(256)                                     # made up, aligned, never dereferenced: a refusal launches nothing
    gv = L.Volumes()
    gv.level[0] = 256
    A = dict(pss=0, i0=0, n=2, packed=one, freq=one, cam=one, u=one, fz=one, up=one, saved=one, cos=one, step=0, g16=one, go16=one, scales=one,
             gmax=one, gin=one, gvols=None, sat=None)

    def call(cfg, **kw):
        a = dict(A, **kw)
        return lib.cnerf_field_chain16(ctypes.byref(cfg), a["pss"], a["i0"], a["n"], a["packed"], a["freq"], a["cam"], a["u"], a["fz"], a["up"], a["saved"],
                                       a["cos"], a["step"], a["g16"], a["go16"], a["scales"], a["gmax"], a["gin"], a["gvols"], a["sat"], None)

    err = lambda: lib.cnerf_last_error()
    cfg = _cfg(L)
    assert call(_cfg(L, kinds=(3, 3, 3))) == -22 and b"per-point FiLM" in err()
    assert call(_cfg(L, precision=L.PREC_FP32)) == -22 and b"FP16X3" in err()
    assert call(_cfg(L, precision=L.PREC_FP16)) == -22 and b"FP16X3" in err()
    for pss in (-1, 3):
        assert call(cfg, pss=pss) == -22 and b"pass" in err()
    for i0, n in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
        assert call(cfg, i0=i0, n=n) == -22 and b"image range" in err(), (i0, n)
    assert call(cfg, step=-1) == -22 and b"group_step" in err()
    for k in ("packed", "up", "saved", "cos", "g16", "go16", "scales", "gmax"):
        assert call(cfg, **{k: None}) == -22 and b"NULL" in err(), k
    assert call(cfg, freq=None) == -22 and b"freq" in err()
    assert call(cfg, cam=None) == -22 and b"cam2world" in err()
    assert call(cfg, pss=1, fz=None) == -22 and b"fine_z" in err()
    assert call(cfg, pss=2, u=None) == -22 and b"points" in err()
    assert call(cfg, gin=one, gvols=ctypes.byref(gv)) == -22 and b"exactly one" in err()
    assert call(cfg, gin=None, gvols=None) == -22 and b"exactly one" in err()
    assert call(cfg, gin=None, gvols=ctypes.byref(L.Volumes())) == -22 and b"gradient volume 0 is NULL" in err()
    assert call(_cfg(L, S=1)) == -22                                  # a cfg that describes no render
