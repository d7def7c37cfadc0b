"""The byte counts of every size entry of the C ABI, pinned to literal numbers.  Callers allocate by these entries and the kernels index
by the same layouts, so a layout that moves by a byte is a change of behaviour; host code only, no GPU.

The numbers in EXPECTED were printed by the library built from the commit BEFORE the host layer was split into csrc/abi_*.hip (the
layouts then lived in one file, csrc/cnerf_abi.hip), by running sizes_of() below against that library -- never by the code under test.
A pull request that changes a layout on purpose replaces the affected numbers and says so."""
import ctypes as C

import pytest

F_HIER, F_SIGMOID, F_XYZ, F_NO_VOLUME = 1, 16, 32, 128
FILM, SINE, RES, PFILM = 0, 1, 2, 3
FP32, FP16, FP16X3 = 0, 1, 2
B = 3           # images; chunks of 2 leave a smaller last chunk

# name -> cfg fields.  R x R = 25 rays and S = 7 samples: 175 points per image, no multiple of the 32-point tile
CASES = {
    "film_fp32": dict(kinds=(FILM,) * 3, precision=FP32),
    "film_fp16x3": dict(kinds=(FILM,) * 3, precision=FP16X3),
    "film_fp16": dict(kinds=(FILM,) * 3, precision=FP16),
    "film_fp32_single_pass": dict(kinds=(FILM,) * 3, precision=FP32, flags=F_SIGMOID),
    "film_fp16x3_single_pass": dict(kinds=(FILM,) * 3, precision=FP16X3, flags=F_SIGMOID),
    "residual_fp32": dict(kinds=(FILM, RES, SINE, RES), precision=FP32, H=128),
    "residual_fp16x3": dict(kinds=(FILM, RES, SINE, RES), precision=FP16X3, H=128),
    "pfilm_fp32": dict(kinds=(PFILM,) * 2, precision=FP32),
    "pfilm_fp16x3": dict(kinds=(PFILM,) * 2, precision=FP16X3),
    "pyramid_fp32": dict(kinds=(FILM,) * 2, precision=FP32, C=96, levels=((8, 32), (4, 32), (2, 32)), flags=F_HIER | F_XYZ),
    "pyramid_fp16x3": dict(kinds=(FILM,) * 2, precision=FP16X3, C=96, levels=((8, 32), (4, 32), (2, 32)), flags=F_HIER | F_XYZ),
    "no_volume_fp32": dict(kinds=(FILM,) * 3, precision=FP32, C=0, V=0, flags=F_HIER | F_NO_VOLUME),
    "no_volume_fp16x3": dict(kinds=(FILM,) * 3, precision=FP16X3, C=0, V=0, flags=F_HIER | F_NO_VOLUME),
    "dropout_fp32": dict(kinds=(FILM,) * 3, precision=FP32, drop_p=0.25),
}


def make_cfg(L, kinds, precision, H=64, C=32, V=8, flags=F_HIER | F_SIGMOID, levels=(), drop_p=0.0):
    cfg = L.Cfg()
    cfg.B, cfg.R, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, 5, 7, V, C, H, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = k
    cfg.n_levels = len(levels)
    for i, (v, c) in enumerate(levels):
        cfg.level_V[i], cfg.level_C[i] = v, c
    cfg.voxel_length, cfg.fov_deg, cfg.flags, cfg.precision, cfg.drop_p = 1.2, 30.0, flags, precision, drop_p
    return cfg


def sizes_of(L, cfg):
    """Every size entry that takes a cfg, in a fixed order; a refusal is recorded as its (negative) return code.
    [packed, fvol_cl, fwd_ws | backward | backward16 | backward_workspace (fp32, fp16) x (chunk B, chunk 2), then fp16 with kept
    activations | field_query_backward_workspace (fp32, fp16) at 1000 points per chunk | pfilm_finish packed_map, workspace (2 images
    of 175 points) | render_rays_workspace (37 rays) | render_rays_backward_workspace (fp32, fp16; 37 rays, 100 points per chunk) |
    render_rays_masked_workspace (37 rays)]"""
    lib, ref = L.lib(), C.byref(cfg)
    out = []

    def call(fn, *args, n_out=1):
        vals = [C.c_size_t(0) for _ in range(n_out)]
        rc = fn(*args, *(C.byref(v) for v in vals))
        out.extend([rc] * n_out if rc else [v.value for v in vals])

    call(lib.cnerf_workspace_bytes, ref, n_out=3)
    call(lib.cnerf_backward_bytes, ref)
    call(lib.cnerf_backward16_bytes, ref)
    for bprec in (FP32, FP16):
        for cnt in (B, 2):
            call(lib.cnerf_backward_workspace_bytes, ref, bprec, cnt, 0)
    call(lib.cnerf_backward_workspace_bytes, ref, FP16, B, 1)
    for bprec in (FP32, FP16):
        call(lib.cnerf_field_query_backward_workspace_bytes, ref, bprec, 1000)
    call(lib.cnerf_pfilm_finish_bytes, ref, 2, 175, n_out=2)
    call(lib.cnerf_render_rays_workspace_bytes, ref, 37)
    for bprec in (FP32, FP16):
        call(lib.cnerf_render_rays_backward_workspace_bytes, ref, bprec, 37, 100)
    call(lib.cnerf_render_rays_masked_workspace_bytes, ref, 37)
    return out


EXPECTED = {
    "film_fp32": [50688, 196608, 153600, 41984, 27136, 1356032, 909824, -22, -22, -22, 3490560, -22, -22, -22, 41216, 409856, -22, 67072],
    "film_fp16x3": [50688, 196608, 173824, 41984, 27136, 1356032, 909824, 875264, 589312, 396032, 3490560, 2353152, -22, -22, 41216, 409856, 328704, 67072],
    "film_fp16": [26112, 196608, 100096, 41984, 27136, 1356032, 909824, -22, -22, -22, 3490560, -22, -22, -22, 41216, 409856, -22, 67072],
    "film_fp32_single_pass": [50688, 196608, 153600, 41984, 27136, 1347584, 901376, -22, -22, -22, 3490560, -22, -22, -22, 41216, 397312, -22, 67072],
    "film_fp16x3_single_pass": [50688, 196608, 173824, 41984, 27136, 1347584, 901376, 866816, 580864, 387584, 3490560, 2353152, -22, -22, 41216, 397312, 316160, 67072],
    "residual_fp32": [364800, 196608, 1090560, 346112, 184832, 5136128, 3429888, -22, -22, -22, 10452992, -22, -22, -22, 41216, 1151488, -22, 67072],
    "residual_fp16x3": [364800, 196608, 1121536, 346112, 184832, 5136128, 3429888, 3017216, 2017280, 1210880, 10452992, 5942528, -22, -22, 41216, 1151488, 821504, 67072],
    "pfilm_fp32": [331008, 196608, 101376, 17408, 158464, 3418112, 2382592, -22, -22, -22, 7223040, -22, 294912, 403200, 41216, 1031936, -22, 67072],
    "pfilm_fp16x3": [331008, 196608, 101376, 17408, 158464, -22, -22, 2694912, 1802496, 1731840, -22, 4639488, -22, -22, 41216, -22, 830208, 67072],
    "pyramid_fp32": [58624, 224256, 175104, 50176, 27136, 1203456, 808192, -22, -22, -22, 3122944, -22, -22, -22, 41216, 387840, -22, 67072],
    "pyramid_fp16x3": [58624, 224256, 196864, 50176, 27136, 1203456, 808192, 1015296, 682752, 572928, 3122944, 2172928, -22, -22, 41216, 387840, 320512, 67072],
    "no_volume_fp32": [50688, 0, 153600, 33792, 27136, 1356032, 909824, -22, -22, -22, 3490560, -22, -22, -22, 41216, 409856, -22, 67072],
    "no_volume_fp16x3": [50688, 0, 173824, 33792, 27136, 1356032, 909824, 807936, 544512, 328704, 3490560, 2353152, -22, -22, 41216, 409856, 328704, 67072],
    "dropout_fp32": [50688, 196608, 153600, 41984, 27136, 1356032, 909824, -22, -22, -22, 3682560, -22, -22, -22, -22, -22, -22, -22],
}

# the size entries that take shapes, not a cfg: (entry, arguments) -> bytes
SHAPE_EXPECTED = {
    ("cnerf_occupancy_compact_bytes", (1, 1)): 256,
    ("cnerf_occupancy_compact_bytes", (3, 175)): 256,
    ("cnerf_occupancy_compact_bytes", (2, 100000)): 512,
    ("cnerf_isosurface_bytes", (2, 2, 2)): 1024,
    ("cnerf_isosurface_bytes", (5, 7, 9)): 3328,
    ("cnerf_isosurface_bytes", (33, 17, 65)): 329728,
    ("cnerf_nearest_points_bytes", (1, 10, 10, 1)): 0,
    ("cnerf_nearest_points_bytes", (1, 100, 100, 0)): 0,
    ("cnerf_nearest_points_bytes", (2, 1000, 5000, 0)): 80384,
    ("cnerf_nearest_points_bytes", (3, 37, 100000, 0)): 87040,
    ("cnerf_nearest_points_bytes", (2, 100, 5000, 4)): 6656,
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_size_entries_of_a_cfg_return_the_pinned_bytes(name):
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    L = cnerf_amd._lib
    assert sizes_of(L, make_cfg(L, **CASES[name])) == EXPECTED[name]


@pytest.mark.parametrize("entry,args", sorted(SHAPE_EXPECTED))
def test_size_entries_of_a_shape_return_the_pinned_bytes(entry, args):
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    lib = cnerf_amd._lib.lib()
    n = C.c_size_t(0)
    assert getattr(lib, entry)(*args, C.byref(n)) == 0, lib.cnerf_last_error()
    assert n.value == SHAPE_EXPECTED[(entry, args)]
