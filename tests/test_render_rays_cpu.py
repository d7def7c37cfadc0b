"""Ray batches (cnerf_render_rays_forward / _backward), no GPU: the host code's exports, workspace sizes and refusals, and the ray
oracle of tests/render_rays_common.py against the reference's own data."""
import ctypes

import numpy as np
import pytest
import torch

import render_rays_common as RC
from oracle import render_oracle as O
from oracle.checks import scaled_err

ENTRIES = ("cnerf_render_rays_workspace_bytes", "cnerf_render_rays_forward", "cnerf_render_rays_backward_workspace_bytes",
           "cnerf_render_rays_backward")
# Distance of the ray oracle's image from the reference's (scaled_err of pixels), the grid's own rays, draws and fine depths given: the
# coarse positions differ from the grid's by ulps (o + d z against the 4x4 transform of a camera-space sample) and the field is
# chaotic in position.  Measured on this oracle; tests/test_gpu_render_rays.py::test_against_the_grid_render uses short_fg_smooth's as
# its floor.
PIXEL_FLOOR = {"short_fg_small": 8.4e-5, "short_fg_smooth": 1.3e-5}


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def rays_cfg(L, kinds=("film",) * 4, precision="fp32", B=2, H=64, S=12):
    cfg = L.Cfg()
    cfg.B, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, S, 8, 32, H, len(kinds)
    for i, k in enumerate(kinds):
        cfg.layer_kind[i] = L.LAYER_CODE[k]
    cfg.voxel_length, cfg.ray_start, cfg.ray_end = 1.2, 0.25, 1.95
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, 8, 32
    cfg.precision = L.PREC_CODE[precision]
    cfg.flags = L.F_HIERARCHICAL
    return cfg                      # R and fov left at 0: a ray batch does not read them


def test_exports_and_prototypes(L):
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10
    assert [f for f, _ in L.Rays._fields_] == ["origins", "dirs"] and ctypes.sizeof(L.Rays) == 16


def fwd_bytes(L, cfg, P):
    n = ctypes.c_size_t()
    return L.lib().cnerf_render_rays_workspace_bytes(ctypes.byref(cfg), P, ctypes.byref(n)), n.value


def bwd_bytes(L, cfg, bprec, P, ppc):
    n = ctypes.c_size_t()
    return L.lib().cnerf_render_rays_backward_workspace_bytes(ctypes.byref(cfg), L.PREC_CODE[bprec], P, ppc, ctypes.byref(n)), n.value


def test_workspace_sizes_grow_with_the_rays_and_with_the_chunk(L):
    cfg = rays_cfg(L)
    sizes = [fwd_bytes(L, cfg, P) for P in (1, 37, 100, 1 << 16)]
    assert all(rc == 0 for rc, _ in sizes), L.lib().cnerf_last_error()
    assert sizes[0][1] < sizes[1][1] < sizes[2][1] < sizes[3][1]
    assert sizes[3][1] >= 2 * (1 << 16) * 12 * (4 + 4 + 1 + 1 + 3) * 4          # both passes' rgb_sigma and z, one pass's positions
    for precision, bprec in (("fp32", "fp32"), ("fp16x3", "fp16")):
        cfg = rays_cfg(L, precision=precision)
        by_rays = [bwd_bytes(L, cfg, bprec, P, 64) for P in (1, 37, 100)]
        by_chunk = [bwd_bytes(L, cfg, bprec, 100, ppc) for ppc in (64, 1000, 1 << 16)]
        assert all(rc == 0 for rc, _ in by_rays + by_chunk), L.lib().cnerf_last_error()
        assert by_rays[0][1] < by_rays[1][1] < by_rays[2][1]
        assert by_chunk[0][1] < by_chunk[1][1] < by_chunk[2][1]
    # no R, no fov: a cfg the grid render refuses
    assert L.lib().cnerf_workspace_bytes(ctypes.byref(rays_cfg(L)), None, None, ctypes.byref(ctypes.c_size_t())) == -22


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    rays = L.Rays()
    rays.origins = rays.dirs = 0x1000
    vols = L.Volumes()
    vols.level[0] = 0x1000

    def forward(cfg, r, P):
        return lib.cnerf_render_rays_forward(ctypes.byref(cfg), ctypes.byref(r) if r is not None else None, P, ctypes.byref(vols), fake, fake, fake, None,
                                             fake, fake, None, fake, None)

    def backward(cfg, r, P):
        sv, fp, gp = L.Saved(), L.FieldParams(), L.FieldParamGrads()
        return lib.cnerf_render_rays_backward(ctypes.byref(cfg), 0, 64, ctypes.byref(r) if r is not None else None, P, ctypes.byref(vols), ctypes.byref(fp),
                                              fake, fake, fake, fake, None, ctypes.byref(sv), fake, None, ctypes.byref(gp), fake, fake, ctypes.byref(vols),
                                              None, None, None, fake, None)

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    no_origins = L.Rays()
    no_origins.dirs = 0x1000
    for call in (forward, backward):
        refused(call(rays_cfg(L), None, 10), "rays is NULL")
        refused(call(rays_cfg(L), no_origins, 10), "origins")
        refused(call(rays_cfg(L), rays, 0), "rays_per_image")
        refused(call(rays_cfg(L, S=1), rays, 10), "S=1")
        refused(call(rays_cfg(L, S=129), rays, 10), "S=129")
        cfg = rays_cfg(L)
        cfg.drop_p = 0.25
        refused(call(cfg, rays, 10), "dropout", "cnerf_render_forward")
    for cfg, P in ((rays_cfg(L, S=1), 10), (rays_cfg(L, S=129), 10), (rays_cfg(L), 0)):
        assert fwd_bytes(L, cfg, P)[0] == -22 and bwd_bytes(L, cfg, "fp32", P, 64)[0] == -22
    # hierarchical sampling without draws, incomplete saved tensors, a backward precision the re-run does not serve: all before a launch
    refused(forward(rays_cfg(L), rays, 10), "u_fine")
    refused(backward(rays_cfg(L), rays, 10), "saved")
    assert bwd_bytes(L, rays_cfg(L, precision="fp32"), "fp16", 10, 64)[0] == -22 and b"fp16x3" in lib.cnerf_last_error()
    assert bwd_bytes(L, rays_cfg(L), "fp32", 10, 0)[0] == -22


@pytest.mark.parametrize("name", ["short_fg_small", "short_fg_smooth"])
def test_ray_oracle_against_the_reference(golden, name):
    """The ray oracle on the grid's own world rays (oracle.render_oracle.coarse_world_points), with the fixture's u_strat, noise draws and
    forced fine depths: coarse_z and fine_points bit-equal to the reference's; the image within the floor recorded above (the coarse
    POSITIONS are not bit-equal: measured 8.4e-5 on short_fg_small -- random volume, x40 density head -- and 1.3e-5 on
    short_fg_smooth, scaled_err of pixels)."""
    g = golden(name)
    m = g.meta
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    B, R, S = m["B"], m["R"], m["S"]
    P = R * R
    cam = T(g["cam2worlds"])
    z_lin, offset, _ = O.stratified_depths(B, R, S, m["ray_start"], m["ray_end"], T(g["u_strat"]))
    grid_pts, dirs_w, org = O.coarse_world_points(cam, O.camera_ray_dirs(R, m["fov"]), z_lin, offset)
    origins = org.reshape(B, 1, 3).expand(B, P, 3).contiguous()
    params = {k: T(v) for k, v in g.params().items()}
    field = RC.oracle_field(m["variant"], params, [T(g["feature_volume"])], T(g["global_feature"]), torch.float32)
    with torch.no_grad():
        px, dist, aux = RC.ray_oracle(field, origins, dirs_w, S, m["ray_start"], m["ray_end"], True, m["clamp"], m["noise"], m["white_back"],
                                      m["last_back"], T(g["u_strat"]), T(g["u_fine"]), T(g.get("eps_coarse")), T(g.get("eps_final")),
                                      forced_fine_z=T(g["fine_z"]))
    assert np.array_equal(aux["coarse_z"].numpy(), g["coarse_z"])
    assert np.array_equal(aux["fine_points"].numpy(), g["fine_points"])
    moved = np.abs(aux["coarse_points"].numpy() - g["coarse_points"]).max()
    assert 0 < moved < 1e-6, moved                       # ulps, and not bit-equal: the floor below is not zero
    ref_px = g["pixels"].reshape(B, 3, P).transpose(0, 2, 1)
    floor = scaled_err(px.numpy(), ref_px)
    print(f"{name}: coarse positions differ by at most {moved:.1e}; ray oracle vs reference pixels: scaled_err {floor:.2e}")
    assert floor <= 1.5 * PIXEL_FLOOR[name], floor       # the recorded number still describes this oracle
    # the ray depth of a grid pixel is the reference's depth over its camera-space z
    dz = O.camera_ray_dirs(R, m["fov"])[:, 2].reshape(1, P)
    assert scaled_err((dist * dz).numpy(), g["depth"].reshape(B, P)) <= max(1e-4, 1.5 * PIXEL_FLOOR[name])
