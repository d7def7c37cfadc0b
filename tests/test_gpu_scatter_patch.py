"""cnerf_scatter_patches -> scatter_sorted_kernel (csrc/scatter_patch.hip), the feature-volume gradient of every half-precision training
step, VOXEL BY VOXEL against float64.

The entry is the production launch (pass_args + launch_scatter_patch, as chunk16 of cnerf_render_backward runs it) fed with rows of the
test's own: random normal fp32, not the chain's.  Every voxel channel of every level must equal base + the float64 scatter of the rows
with the float64 trilinear weights of the float32 sample positions (those cnerf_render_forward reports for the same u_strat / fine_z)
within the derived bound of tests/scatter_patch_common.py; a zero bound (no sample point near the voxel: half of the 40^3 case)
demands the base bit for bit.  tests/test_scatter_patch_cpu.py shows that an honest float32 implementation attains the bound, that
every case reaches the path it is named for, and that each hazard -- a dropped tail, a batch processed twice, a clamped +1 corner with
its twin's weight, the rows of the neighbouring image or feature tile, a window origin off by one, an unmasked last quad, a run split
between half-waves added once -- exceeds it.

Buffers: CANARY rows of 1e30 behind the last row of gin (a read there makes an output non-finite); B + 1 image slots per gradient
volume, the slots outside the chunk hold a sentinel; the chunk's slots start from a non-zero random base (the entry accumulates).  A
second call adds the same again: base + 2 x the float64 scatter within 4 x the bound (the first call's, the second sum's own, and
adding it onto a partial result of that size).

scatter_sorted_kernel, -Rpass-analysis=kernel-resource-usage of the gfx950 build:
    TotalSGPRs: 106   VGPRs: 152   AGPRs: 0   ScratchSize: 0   Occupancy [waves/SIMD]: 3   SGPRs Spill: 78   VGPRs Spill: 0
    LDS Size [bytes/block]: 0 static + 53616 dynamic (rows 32768, records 16384, counts 2048, queue 2048, misc 16, corners 96, outside 256)

Measured worst |err| / bound per case (MI355X), first call / second call (against 4 x the bound):
    coarse_sparse_v40   0.687 / 0.344     fine_tail_44       0.050 / 0.025     pyramid_coarse  0.037, 0.005, 0.001 / 0.018, 0.003, 0.000 (levels 0, 1, 2)
    coarse_one_window   0.004 / 0.002     fine_ring_1536     0.020 / 0.010     pyramid_fine    0.045, 0.005, 0.001 / 0.023, 0.002, 0.000
    coarse_image_range  0.722 / 0.361     fine_second_round  0.006 / 0.003     dgx_coarse 0.033 / 0.017   dgx_fine 0.037 / 0.019   one-hot 0.096 / 0.048
The two sparse volumes come close to the bound exactly as the honest float32 emulation does on the CPU (0.75, 0.78): a voxel with ONE
addend a on a base b may err by 4 u |a| + u |b| of the 5 u |a| + u |b| allowed; where tens of addends meet, rounding errors average out.
No derived term had to be corrected on the hardware; the one term beyond scatter64's, k u |base|, was derived before the first run
(tests/scatter_patch_common.py).  The positions the forward reported were bit-identical to their float32 NumPy restatement in every case
(printed, not asserted), so the populations and window paths test_scatter_patch_cpu.py asserts are those the kernel ran.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import field_backward_stage_common as S
import scatter_patch_common as P
from test_gpu_pfilm_finish import within

pytestmark = pytest.mark.gpu

CANARY = 4
SENT = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def run_scatter(dev, name, one_hot=False):
    """One case of scatter_patch_common.CASES through cnerf_scatter_patches, twice; returns (inputs, [(want, bound, k)], volumes after
    the first call) of the chunk's images."""
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    lib = L.lib()
    c = P.case_inputs(name, one_hot)
    B, R, Sn, pss, image0, n_images = (c[k] for k in ("B", "R", "S", "pss", "image0", "n_images"))
    npi = R * R * Sn
    net, _ = S.make_net(c["variant"], 64, 11)
    g = torch.Generator().manual_seed(3)
    freq = phase = None
    if net.spec.has_global:
        with torch.no_grad():
            freq, phase = (t.to(dev).contiguous() for t in net.film(torch.randn((B, S.Z_DIM), generator=g)))
    net.to(dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vols = [(torch.randn((B, v, v, v, ch), generator=g) * 0.5).to(dev) for v, ch in c["levels"]]
    cam, u_strat = T(c["cams"]), T(c["u_strat"]).reshape(B, R * R, Sn)
    fine_z = T(c["fine_z"] if pss == 1 else 0.25 + 1.7 * np.random.default_rng(1).random((B, npi), dtype=np.float32)).reshape(B, R * R, Sn)
    # the positions cnerf_render_forward reports for the same u_strat / fine_z
    aux = ops.render_forward(net, vols, freq, phase, cam, R, P.FOV, P.RAY_START, P.RAY_END, Sn, True, "relu", 0.0,
                             rng=dict(u_strat=u_strat, u_fine=torch.rand((B, R * R, Sn), device=dev), fine_z=fine_z), fvol_is_channel_last=True,
                             aux_keys=("coarse_points", "fine_points"))[2]
    pts = aux[("coarse", "fine")[pss] + "_points"].reshape(B, npi, 3)[image0:image0 + n_images].cpu().numpy()
    assert np.isfinite(pts).all()
    geom = P.Geom(R, Sn)
    draws = (c["fine_z"] if pss == 1 else c["u_strat"])[image0:image0 + n_images]
    twin = np.stack([geom.positions(pss, m, d, np.arange(npi)) for m, d in zip(c["cams"][image0:image0 + n_images], draws)])
    print(f"{name}: positions of the forward vs their float32 NumPy restatement: max |diff| {np.abs(twin - pts).max():.1e}, "
          f"{(twin != pts).mean() * 100:.2f} % of the coordinates differ")
    cfg = ops.make_cfg(net, B, vols, R, Sn, precision="fp32", ray_start=P.RAY_START, ray_end=P.RAY_END, fov=P.FOV, hierarchical=True)
    assert [(int(cfg.level_V[i]), int(cfg.level_C[i])) for i in range(cfg.n_levels)] == c["levels"]

    gin = torch.cat([T(c["gin"]).reshape(-1, 32), torch.full((CANARY, 32), 1e30, device=dev)]).contiguous()
    gvols = [torch.full((B + 1, v, v, v, ch), SENT, device=dev) for v, ch in c["levels"]]
    for gv, b in zip(gvols, c["base"]):
        gv[image0:image0 + n_images] = T(b)
    gvs = ops.volumes_struct(gvols)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        L.check(lib.cnerf_scatter_patches(C.byref(cfg), pss, image0, n_images, L.ptr(cam), L.ptr(u_strat), L.ptr(fine_z), L.ptr(gin), C.byref(gvs), stream),
                "cnerf_scatter_patches")
        torch.cuda.synchronize()
        outside = [b for b in range(B + 1) if not image0 <= b < image0 + n_images]
        for gv in gvols:
            assert (gv[outside] == SENT).all(), "a gradient volume slot outside the chunk was written"
        got = [gv[image0:image0 + n_images].cpu().numpy() for gv in gvols]
        assert all(np.isfinite(a).all() for a in got), "a canary row was read"
        return got

    exp = P.expected(c["gin"], pts, c["tiles"], c["base"])
    first = call()
    for lvl, ((want, bound, _), got) in enumerate(zip(exp, first)):
        assert np.abs(want - c["base"][lvl]).max() > 0
        within(got, want, bound, f"{name} level {lvl}")
    second = call()
    for lvl, ((want, bound, _), got) in enumerate(zip(exp, second)):
        within(got, 2.0 * want - c["base"][lvl].astype(np.float64), 4.0 * bound, f"{name} twice level {lvl}")
    return c, exp, first


@pytest.mark.parametrize("name", list(P.CASES))
def test_every_voxel_against_float64(dev, name):
    """coarse_sparse_v40: pixels several voxels apart, most points outside the window; ragged patches (96-point batch, 36 points direct),
    a 2-sample last quad.  coarse_one_window: full batches inside one window, runs split between half-waves, clamped +1 corners.
    coarse_image_range: images [1, 3) of 3.  fine_tail_44: unsorted depths, a batch and a direct tail of 44, a partial batch of 212,
    256 | 256.  fine_ring_1536: six batches of one bin through the 512-slot ring, depths beyond the ray's ends.  fine_second_round: 18
    quads, the second round of 16.  pyramid_* / dgx_*: four feature tiles on three levels (in_chan 0 and 32 of the 64-channel level);
    one feature tile beside an xyz tile without rows."""
    c, exp, first = run_scatter(dev, name)
    if name == "coarse_sparse_v40":
        zero = exp[0][1] == 0
        assert zero.mean() > 0.45 and np.array_equal(first[0][zero], c["base"][0][zero])


def test_one_hot_rows_change_only_their_corners(dev):
    """A single non-zero row per image in the 40^3 volume: at most the 8 corners of that point change, all of them inside its 4^3
    neighbourhood, and every other voxel channel keeps its base bit for bit."""
    c, exp, first = run_scatter(dev, "coarse_sparse_v40", one_hot=True)
    (want, bound, _), base = exp[0], c["base"][0]
    changed = (first[0] != base).any(axis=-1)
    near = (bound > 0).any(axis=-1)
    per_image = changed.reshape(c["n_images"], -1).sum(axis=1)
    assert ((per_image >= 1) & (per_image <= 8)).all(), per_image
    assert not (changed & ~near).any()
    assert (near.reshape(c["n_images"], -1).sum(axis=1) <= 64).all()
