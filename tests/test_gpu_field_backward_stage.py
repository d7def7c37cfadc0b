"""cnerf_field_backward / cnerf_field_backward_points: the stage every fp32 parameter gradient is a GEMM or column sum over -- the
activation-storing re-run (field_tile_kernel / field_pw_kernel, STORE), the gradient chain (field_backward_kernel /
field_pw_backward_kernel) and its in-kernel volume scatter -- ROW BY ROW against float64.

The formulas, bounds and their derivations are in tests/field_backward_stage_common.py (tests/test_field_backward_stage_cpu.py shows
that an honest float32 implementation attains them and that each hazard below exceeds them).  Every element of every output slab is
compared, each step from the rows the stage itself stored one step earlier; a zero bound demands equality.  What the cases are for:
padded lanes that shadow an image's last point (ragged shapes), `valid`, one image reading its neighbour's freq (per-image freq, image0),
a drop_gp that forgets image0 (dropout from image 1, injected and Philox), the slabs of a residual block, every input-tile layout, and
the tile a wave handles second.

Buffers: CANARY rows of 1e30 behind the last row of every per-point input (a read there makes an output non-finite), a sentinel behind
every act_* output, in one image slot behind the gradient volumes and in the slots of the images outside the chunk.  A second call on
the same buffers must leave every act_* row bit-identical and double the volumes (within 4 x their bound: the second sum's own bound,
and adding it onto a base of that size).

A wave's second tile: field_backward_kernel<8, false, false> and field_tile_kernel<8, false, true, false, false, 0, false> (H = 256,
STORE) both report, from -Rpass-analysis=kernel-resource-usage of the gfx950 build,
    VGPRs: 256   AGPRs: 164 / 206   Occupancy [waves/SIMD]: 1   LDS Size [bytes/block]: 25088 / 32768
(field_pw_backward_kernel<8>: VGPRs 214, AGPRs 128, occupancy 1): one 256-thread block per CU, so the grid of field_grid() is at most
256 blocks x 4 waves on the 256 CUs and every eighth of the tiles is walked by 128 waves.  2 images x 24576 points = 1536 tiles = 192
per band: 64 waves of each band own two tiles, 64 one.

Measured worst |err| / bound per check over all cases (MI355X):
    act_feat 0.11 (xyz tile: equal)   act_h / act_c 0.30 / 0.29 (layer 0 of SHORTSIREN's three fmas; FiLM and sine slabs below 0.12)
    residual fc1 / fc2: act_h 0.12 / 0.10, act_c 0.09 / 0.11   per-point FiLM: m 0.12, y 0.04, cos / cos freq / cos 15 pre 0.04 / 0.04 / 0.07
    act_go 0.80   act_g 0.42 (the head's 4-term product; lower slabs 0.06)   g_pre / G freq / G phase 0.34 / 0.31 / 0.31
    gradient volumes 0.03, second call 0.002
No derived term had to be corrected on the hardware.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import field_backward_stage_common as S

pytestmark = pytest.mark.gpu

CANARY = 4
SENT = 12345.0
TAIL = 256          # sentinel floats behind every act_* buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def _with_canary(t, dev):
    """t (rows, w) on the device with CANARY rows of 1e30 behind its last row."""
    t = torch.from_numpy(np.ascontiguousarray(t)).reshape(-1, t.shape[-1])
    return torch.cat([t, torch.full((CANARY, t.shape[1]), 1e30)]).to(dev).contiguous()


def run_stage(dev, variant, H, B, npi, *, precision="fp32", entry="points", image0=0, n_images=None, drop_p=0.0, philox_drop=False,
              R=0, S_=0, seed=0, forward=True):
    """One stage call (twice) on random inputs and every check of tests/field_backward_stage_common.py."""
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    lib = L.lib()
    n_images = B if n_images is None else n_images
    net, levels = S.make_net(variant, H, 1000 * H + npi + seed)
    sn = S.stage_net(net)
    case = S.random_case(net, levels, B, npi, 77 + seed, drop_p)
    net.to(dev)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vols = [T(v) for v in case.levels]
    freq, phase = T(case.freq), T(case.phase)
    drop = (drop_p, (0x1234ABCD5678, 9)) if drop_p else None
    cfg = ops.make_cfg(net, B, vols if vols else [], max(R, 1), max(S_, 2), precision=precision, drop=drop, ray_start=0.25, ray_end=1.95, fov=49.13,
                       hierarchical=entry in ("coarse", "fine"))
    packed, packed_t = ops.pack_field(net, cfg), ops.pack_field_transposed(net, cfg)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vs = ops.volumes_struct(vols)
    cam = u_strat = fine_z = None
    if entry in ("coarse", "fine"):        # the positions cnerf_render_forward reports for the same u_strat / fine_z
        from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
        assert R * R * S_ == npi
        torch.manual_seed(seed + 5)
        cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y").to(dev).contiguous()
        u_strat, u_fine = torch.rand((B, R * R, S_), device=dev), torch.rand((B, R * R, S_), device=dev)
        fine_z = (0.25 + 1.7 * torch.rand((B, R * R, S_), device=dev)).contiguous()
        aux = ops.render_forward(net, vols, freq, phase, cam, R, 49.13, 0.25, 1.95, S_, True, "relu", 0.0, rng=dict(u_strat=u_strat, u_fine=u_fine, fine_z=fine_z),
                                 fvol_is_channel_last=True, aux_keys=("coarse_points", "fine_points"))[2]
        case.points = aux[entry + "_points"].reshape(B, npi, 3).cpu().numpy()
        assert np.isfinite(case.points).all() and (np.abs(case.points) > 0.6).any() and (np.abs(case.points) < 0.6).any()
    pts = _with_canary(case.points, dev)
    saved = torch.full((B * npi + CANARY, 4), 1e30, device=dev)
    L.check(lib.cnerf_field_forward(C.byref(cfg), C.byref(vs), L.ptr(packed), L.ptr(freq), L.ptr(phase), L.ptr(pts), npi, L.ptr(saved), stream),
            "cnerf_field_forward")
    torch.cuda.synchronize()
    case.saved = saved[:B * npi].reshape(B, npi, 4).cpu().numpy()
    assert np.isfinite(case.saved).all() and (saved[B * npi:] == 1e30).all()
    up = _with_canary(case.upstream, dev)

    chunk = S.chunk_of(case, image0, n_images)
    n = n_images * npi
    mask = None
    if drop_p and not philox_drop:
        mask = T(case.drop[1])             # the FULL (n_drop, B, npi, H) tensor
    elif drop_p:                           # the decisions the kernels draw themselves (stream 6), as cnerf_dropout_keep reports them
        keep = torch.empty((case.drop[1].shape[0], n, H), dtype=torch.uint8, device=dev)
        L.check(lib.cnerf_dropout_keep(C.byref(cfg), 6, image0 * npi, n, L.ptr(keep), stream), "cnerf_dropout_keep")
        torch.cuda.synchronize()
        chunk.drop = (chunk.drop[0], keep.reshape(-1, n_images, npi, H).cpu().numpy())
        frac = float(keep.float().mean())
        assert abs(frac - (1 - drop_p)) < 0.02, frac

    sizes = dict(zip(("act_feat", "act_h", "act_c", "act_g", "act_go"), S.act_sizes(sn, n, case.levels)))
    act = {k: torch.full((sz + TAIL,), SENT, device=dev) for k, sz in sizes.items()}
    gvols = [torch.full((B + 1,) + tuple(v.shape[1:]), SENT, device=dev) for v in vols]
    for g in gvols:
        g[image0:image0 + n_images] = 0.0
    gvs = ops.volumes_struct(gvols)
    novol = sn.input == "position"

    def call():
        tail = (L.ptr(up), L.ptr(saved), L.ptr(act["act_feat"]), L.ptr(act["act_h"]), L.ptr(act["act_c"]), L.ptr(act["act_g"]), L.ptr(act["act_go"]),
                None if novol else C.byref(gvs), L.ptr(mask), stream)
        v = None if novol else C.byref(vs)
        if entry == "points":
            assert image0 == 0 and n_images == B
            rc = lib.cnerf_field_backward_points(C.byref(cfg), v, L.ptr(packed), L.ptr(packed_t), L.ptr(freq), L.ptr(phase), L.ptr(pts), npi, *tail)
        else:
            if cam is None:
                eye = torch.eye(4, device=dev).repeat(B, 1, 1).contiguous()
            pss = {"coarse": 0, "fine": 1, "pass2": 2}[entry]
            rc = lib.cnerf_field_backward(C.byref(cfg), pss, image0, n_images, v, L.ptr(packed), L.ptr(packed_t), L.ptr(freq), L.ptr(phase),
                                          L.ptr(cam if cam is not None else eye), L.ptr(pts if pss == 2 else u_strat), L.ptr(fine_z), *tail)
        L.check(rc, "cnerf_field_backward" + ("_points" if entry == "points" else ""))
        torch.cuda.synchronize()

    def sentinels_intact():
        for k, sz in sizes.items():
            assert (act[k][sz:] == SENT).all(), k
        for g in gvols:
            outside = [b for b in range(B + 1) if not image0 <= b < image0 + n_images]
            assert (g[outside] == SENT).all(), "a gradient volume slot outside the chunk was written"

    call()
    sentinels_intact()
    out = {k: act[k][:sz].cpu().numpy() for k, sz in sizes.items()}
    out["grad_vols"] = [g[image0:image0 + n_images].cpu().numpy() for g in gvols]
    for k, v in out.items():
        assert all(np.isfinite(a).all() for a in (v if isinstance(v, list) else [v])), k     # nothing came from a canary row
    tag = f"{variant} {H} {entry} "
    if forward:
        assert precision == "fp32"
        S.check_forward_rows(sn, chunk, out, tag)
    expect = S.check_chain_rows(sn, chunk, out, tag)
    if sn.pfilm:                               # this family's scatter belongs to cnerf_pfilm_backward_finish: grad_vols is not touched
        assert all((g[image0:image0 + n_images] == 0).all() for g in gvols)

    call()
    sentinels_intact()
    for k, sz in sizes.items():
        assert np.array_equal(act[k][:sz].cpu().numpy(), out[k]), f"{k} differs between two calls on the same inputs"
    for lvl, (g, (_, bound)) in enumerate(zip(gvols, expect)):
        S.within(g[image0:image0 + n_images], 2.0 * out["grad_vols"][lvl].astype(np.float64), 4.0 * bound, f"{tag}twice grad volume {lvl}")


@pytest.mark.parametrize("B,npi,H", [(1, 1, 64), (2, 45, 64), (1, 33, 128), (3, 70, 256)])
def test_every_width_and_ragged_tiles(dev, B, npi, H):
    """A single partial tile; ragged tiles across image boundaries (per-image freq on either side); every width."""
    run_stage(dev, "SHORTSIREN_FG", H, B, npi)


KINDS = ["SHORTSIREN_F", "SHORTSIREN_FRes", "TALLSIREN_dResLong", "SingleSIREN_dg", "TALLSIREN_dgx", "SHORTSIREN_FG_Pyrmd", "SHORTSIREN", "TALLSIREN"]


@pytest.mark.parametrize("variant,H", [(v, 64) for v in KINDS] + [(v, 256) for v in ("TALLSIREN_dgx", "SHORTSIREN_FRes", "SHORTSIREN", "TALLSIREN")])
def test_layer_kinds(dev, variant, H):
    """Sine layers; one and four residual blocks (two slabs each, the identity term); L = 1 (no transposed product); two input tiles
    whose xyz columns get no scatter; several levels; no volume at all (NULL volumes); the per-point FiLM family."""
    run_stage(dev, variant, H, 2, 45)


def test_image_range(dev):
    """Images [1, 3) of a call of 3: per-image freq, the rows of upstream / saved, the positions and the volume slots all start at
    image 1; slot 0 of the gradient volumes is untouched."""
    run_stage(dev, "SHORTSIREN_FG", 64, 3, 45, entry="pass2", image0=1, n_images=2, R=3, S_=5)


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "TALLSIREN_dgx"])
@pytest.mark.parametrize("entry", ["coarse", "fine"])
def test_ray_passes(dev, entry, variant):
    """Image 1 of 2: the kernels form the sample positions themselves (camera, u_strat / fine_z of that image); act_feat is held to the
    positions cnerf_render_forward reports (the xyz tile of TALLSIREN_dgx: bit for bit)."""
    run_stage(dev, variant, 64, 2, 45, entry=entry, image0=1, n_images=1, R=3, S_=5)


@pytest.mark.parametrize("philox_drop", [False, True], ids=["injected", "philox"])
@pytest.mark.parametrize("variant", ["SHORTSIREN_FRes", "TALLSIREN"])
def test_dropout(dev, variant, philox_drop):
    """p = 0.3 on image 1 of 2: the stored rows are the eval-mode rows times keep / (1 - p), a dropped element exactly zero; the keep
    decisions are those of image 1 in the FULL injected tensor, or (drop_mask = NULL) Philox stream 6 at the point's index in the whole
    call, as cnerf_dropout_keep reports them."""
    run_stage(dev, variant, 256, 2, 45, entry="pass2", image0=1, n_images=1, drop_p=0.3, philox_drop=philox_drop, R=3, S_=5)


@pytest.mark.parametrize("variant", ["SHORTSIREN_FG", "SHORTSIREN_FRes"])
def test_fp16x3_rerun(dev, variant):
    """The re-run in split precision stores the rows; the chain and the scatter are fp32 and layer-local, so their bounds do not move."""
    run_stage(dev, variant, 256, 2, 45, precision="fp16x3", forward=False)


def test_second_tile_of_a_wave(dev):
    """1536 tiles in the call: within every band 64 waves own two tiles and 64 exactly one (module docstring)."""
    run_stage(dev, "SHORTSIREN_FG", 256, 2, 24576)
