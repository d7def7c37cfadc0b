"""What tests/test_gpu_scatter_patch.py holds scatter_sorted_kernel to, checked without a GPU (tests/scatter_patch_common.py):

1. Partition.  The float32 restatement of the block decomposition claims every point of every image of every case exactly once, and
   the cases reach the paths they are named for: the populations asserted below, no fine depth within 1e-4 of a bin edge (so a depth
   cannot change its bin by a rounding the restatement does not share with the kernel).
2. An honest float32 emulation of the algorithm -- records sorted by voxel, sequential run sums, one add per run and half-wave, direct
   adds outside the window and for tails of 48 points or fewer, onto a non-zero base -- stays inside the bound on every case: the
   bound is attainable.  Worst |err| / bound per case: 0.75 and 0.78 in the sparse volumes (V = 40, 24: a voxel with ONE addend a on a
   base b may err by 4 u |a| + u |b| of the 5 u |a| + u |b| allowed), 0.003 - 0.10 where voxels sum tens of addends.
3. Each hazard of the kernel, applied to the emulation, exceeds the bound at some voxel of the case named for it.
4. cnerf_scatter_patches refuses pass 2, a network without a volume, NULL arguments and image ranges outside [0, B) with CNERF_EINVAL
   on the host (nothing is launched: the addresses are made up)."""
import ctypes
import os

import numpy as np
import pytest

import scatter_patch_common as P
from test_gpu_pfilm_finish import within


def _points(c):
    """Positions (n_images, npi, 3) float32 of the chunk's images, and their draws (n_images, npi)."""
    geom = P.Geom(c["R"], c["S"])
    sl = slice(c["image0"], c["image0"] + c["n_images"])
    draws = (c["fine_z"] if c["pss"] == 1 else c["u_strat"])[sl]
    nn = np.arange(c["R"] * c["R"] * c["S"])
    return geom, np.stack([geom.positions(c["pss"], m, d, nn) for m, d in zip(c["cams"][sl], draws)]), draws


@pytest.fixture(scope="module")
def honest():
    """Per case (inputs, geometry, positions, draws, expectation, the honest emulation's volumes): computed once, never modified."""
    out = {}
    for name in P.CASES:
        c = P.case_inputs(name)
        geom, pts, draws = _points(c)
        sl = slice(c["image0"], c["image0"] + c["n_images"])
        out[name] = (c, geom, pts, draws, P.expected(c["gin"], pts, c["tiles"], c["base"]),
                     P.emulate(geom, c["pss"], c["cams"][sl], draws, c["gin"], c["tiles"], c["base"]))
    return out


def _check(c, exp, vols, tag):
    for lvl, ((want, bound, _), got) in enumerate(zip(exp, vols)):
        within(got, want, bound, f"{tag} level {lvl}")


def test_every_point_is_claimed_once_and_the_cases_reach_their_paths():
    sizes = {}
    for name, (variant, B, R, S, V, pss, image0, n_images) in P.CASES.items():
        c = P.case_inputs(name)
        geom = P.Geom(R, S)
        assert geom.NQ == (S + 3) // 4
        for b in range(B):
            z = c["fine_z"][b] if pss == 1 else None
            pop = P.populations(geom, pss, z)                      # asserts the partition
            assert sum(n for w in pop.values() for _, n in w) == R * R * S
            sizes[name, b] = pop
            if pss == 1:
                q, edge = geom.depth_bin(z)
                assert edge.min() > 1e-4, (name, b, edge.min())
                assert (np.diff(z.reshape(R * R, S), axis=1) < 0).any(axis=1).all(), "depths unsorted along every ray"
    # coarse, R = 11, S = 10: NQ = 3 with a 2-sample last quad; patches of 8 x 8, 8 x 3, 3 x 8 and 3 x 3 rays
    pop = sizes["coarse_sparse_v40", 0]
    assert pop[0, 0, 0] == [("batch", 256)] and pop[0, 1, 0] == [("batch", 96)] and pop[1, 1, 0] == [("direct", 36)]
    assert pop[0, 0, 2] == [("batch", 128)] and pop[1, 1, 2] == [("direct", 18)]
    assert sizes["coarse_one_window", 0] == {(0, 0, 0): [("batch", 256)], (0, 0, 1): [("batch", 256)]}
    assert sizes["coarse_image_range", 1][1, 1, 1] == [("direct", 1)]                         # S = 5: sample 4 of the one ray of patch (1, 1)
    # fine, NQ = 2: 300 = a batch and a direct tail of 44; 212 = a partial batch; 256 | 256 = no tail
    assert sizes["fine_tail_44", 1] == {(0, 0, 0): [("batch", 256), ("direct", 44)], (0, 0, 1): [("batch", 212)]}
    assert sizes["fine_tail_44", 2] == {(0, 0, 0): [("batch", 256)], (0, 0, 1): [("batch", 256)]}
    # fine, NQ = 6: 1536 points of one bin through the 512-slot ring, six full batches; depths beyond the ray's ends clamp to bins 0 and 5
    pop = sizes["fine_ring_1536", 0]
    assert pop[0, 0, 2] == [("batch", 256)] * 6 and all(pop[0, 0, q] == [] for q in (0, 1, 3, 4, 5))
    pop = sizes["fine_ring_1536", 1]
    assert pop[0, 0, 0] == [("batch", 256)] * 3 + [("direct", 32)] and pop[0, 0, 5] == [("batch", 256)] * 2 + [("batch", 224)]
    assert all(pop[0, 0, q] == [] for q in (1, 2, 3, 4))
    g = P.Geom(8, 24)
    assert (g.depth_bin(np.float32([0.02, 0.2, 2.0, 2.2]))[0] == [0, 0, 5, 5]).all() and 0.2 < P.RAY_START and 2.0 > P.RAY_END
    # fine, NQ = 18: the quads of a ray are walked in two rounds of 16 and 2; every bin is populated, from samples of both rounds
    pop = sizes["fine_second_round", 0]
    assert len(pop) == 18 and all(sum(n for _, n in w) > 100 for w in pop.values())
    c = P.case_inputs("fine_second_round")
    q = P.Geom(8, 72).depth_bin(c["fine_z"][0])[0].reshape(64, 72)
    assert all((q[:, :64] == b).any() and (q[:, 64:] == b).any() for b in range(18))
    # several feature tiles: four for the pyramid (the 64-channel level: channels 0 and 32), one for TALLSIREN_dgx (its xyz tile has no rows)
    assert P.level_shapes("SHORTSIREN_FG_Pyrmd", 12) == ([(12, 32), (6, 64), (3, 32)], [(0, 0), (1, 0), (1, 32), (2, 0)])
    assert P.level_shapes("TALLSIREN_dgx", 12) == ([(12, 32)], [(0, 0)])


def test_window_paths_of_the_cases(honest):
    """Pixels several voxels apart (V = 40): most points of a batch have a corner outside the 8^3 window; R = 8 in V = 6 (at V = 12 the
    one patch, the whole image, outgrows the window: a third of its points inside): all or nearly all points inside, runs of ~10 records on the
    <= 216 voxels, split between half-waves, and clamped +1 corners where the rays (0.25 - 1.95) leave the cube."""
    def inside_fraction(name):
        c, geom, pts, draws, _, _ = honest[name]
        n_in = n_all = clamped = 0
        for b in range(c["n_images"]):
            m = c["cams"][c["image0"] + b]
            for pr, pc, q, work in P.blocks(geom, c["pss"], draws[b] if c["pss"] == 1 else None):
                o = geom.window_origin(c["pss"], m, pr, pc, q, c["V"])
                for kind, nn in work:
                    if kind != "batch":
                        continue
                    i0 = P.unnormalize(pts[b][nn], c["V"])[0]
                    one = (i0 + 1 < c["V"]).astype(np.int64)
                    ins = ((i0 - o >= 0) & (i0 - o + one < P.BOX)).all(axis=1)
                    n_in, n_all, clamped = n_in + ins.sum(), n_all + len(nn), clamped + (ins & (one == 0).any(axis=1)).sum()
        return n_in / n_all, clamped
    frac, _ = inside_fraction("coarse_sparse_v40")
    assert 0.0 < frac < 0.5, frac
    frac, clamped = inside_fraction("coarse_one_window")
    # (not all: the rays are normalised, so the far samples of a patch's central rays lie beyond the hull of its 8 frustum corners and
    # may fall below the window's origin -- they are added directly, by design; which few do depends on the camera to the ulp)
    assert frac > 0.95 and clamped > 20, (frac, clamped)


@pytest.mark.parametrize("name", list(P.CASES))
def test_honest_float32_emulation_stays_inside_the_bound(honest, name):
    c, _, _, _, exp, vols = honest[name]
    _check(c, exp, vols, name)
    for want, bound, k in exp:
        assert (bound[np.broadcast_to(k == 0, bound.shape)] == 0).all() and np.abs(want).max() > 0
    if name == "coarse_sparse_v40":                               # half of the 40^3 volume: untouched, equality demanded
        assert (exp[0][1] == 0).mean() > 0.45


#            hazard                          the case named for it
HAZARD_CASE = {"dropped_tail": "fine_tail_44", "batch_twice": "fine_ring_1536", "clamped_twin": "coarse_one_window",
               "image0_rows": "coarse_image_range", "tile0_rows": "pyramid_fine", "origin_off_by_one": "coarse_one_window",
               "unmasked_last_quad": "coarse_sparse_v40", "run_across_half_waves_once": "coarse_one_window"}


@pytest.mark.parametrize("hazard", P.HAZARDS)
def test_hazard_exceeds_the_bound(honest, hazard):
    c, geom, _, draws, exp, vols = honest[HAZARD_CASE[hazard]]
    sl = slice(c["image0"], c["image0"] + c["n_images"])
    bad = P.emulate(geom, c["pss"], c["cams"][sl], draws, c["gin"], c["tiles"], c["base"], hazard=hazard)
    assert any(not np.array_equal(a, b) for a, b in zip(bad, vols))
    with pytest.raises(AssertionError, match="level"):
        _check(c, exp, bad, hazard)


def test_one_hot_rows_touch_eight_voxels(honest):
    """One non-zero row per image: the bound is zero (equality with the base) everywhere but at that point's 4^3 neighbourhood, and
    the float64 scatter differs from the base at no more than 8 voxels per image."""
    c = P.case_inputs("coarse_sparse_v40", one_hot=True)
    _, _, pts, _, _, _ = honest["coarse_sparse_v40"]
    (want, bound, _), = P.expected(c["gin"], pts, c["tiles"], c["base"])
    changed = (want != c["base"][0].astype(np.float64)).any(axis=-1).reshape(c["n_images"], -1).sum(axis=1)
    assert ((changed >= 1) & (changed <= 8)).all(), changed
    assert ((bound > 0).any(axis=-1).reshape(c["n_images"], -1).sum(axis=1) <= 64).all()


def _cfg(L, B=2, R=6, S=10, V=8, flags=0, C=32):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, R, S, V, C, 64, 4
    cfg.voxel_length, cfg.fov_deg, cfg.flags, cfg.ray_start, cfg.ray_end = 1.2, 30.0, flags, 0.25, 1.95
    return cfg


def test_entry_refuses_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    lib = L.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(ge.__file__)), "include", "cnerf.h")).read()
    assert "int cnerf_scatter_patches(" in header and "#define CNERF_ABI_VERSION 10" in header and lib.cnerf_abi_version() == 10
    one = ctypes.c_void_p(256)                                     # made up, aligned, never dereferenced: a refusal launches nothing
    gv = L.Volumes()
    gv.level[0] = 256
    cfg = _cfg(L, flags=L.F_SIGMOID_RGB | L.F_HIERARCHICAL)
    call = lambda cfg, pss, i0, n, cam=one, u=one, fz=one, gin=one, g=ctypes.byref(gv): lib.cnerf_scatter_patches(
        ctypes.byref(cfg), pss, i0, n, cam, u, fz, gin, g, None)
    err = lambda: lib.cnerf_last_error()
    assert call(cfg, 2, 0, 2) == -22 and b"pass" in err()
    assert call(cfg, -1, 0, 2) == -22 and b"pass" in err()
    for i0, n in ((-1, 1), (0, 0), (0, 3), (2, 1), (1, 2)):
        assert call(cfg, 0, i0, n) == -22 and b"image range" in err(), (i0, n)
    assert call(cfg, 0, 0, 2, cam=None) == -22 and b"NULL" in err()
    assert call(cfg, 0, 0, 2, gin=None) == -22 and b"NULL" in err()
    assert call(cfg, 0, 0, 2, g=None) == -22 and b"NULL" in err()
    assert call(cfg, 1, 0, 2, fz=None) == -22 and b"fine_z" in err()
    assert call(cfg, 0, 0, 2, g=ctypes.byref(L.Volumes())) == -22 and b"gradient volume 0 is NULL" in err()
    nv = _cfg(L, V=0, C=0, flags=L.F_NO_VOLUME | L.F_SIGMOID_RGB | L.F_HIERARCHICAL)
    assert call(nv, 0, 0, 2) == -22 and b"NO_VOLUME" in err()
    assert call(_cfg(L, S=1), 0, 0, 2) == -22                        # a cfg that describes no render
