"""cnerf_field_chain16: the half-precision gradient chain (chain16_kernel<NT, DRY, HAS_RES>, csrc/bwd16.hip) with the launches the
render runs around it -- head scale, dry run over the sampled tile groups, per-slab scales, chain -- ROW BY ROW against float64.

The formulas, the bounds and their derivations are in tests/chain16_common.py; tests/test_chain16_cpu.py shows that an honest float32
emulation attains them and that each named hazard exceeds them or breaks an equality.  Every element of go16, of every slab of g16 and
of the layer-0 rows gin (or the gradient volumes the chain adds to itself) is compared, each step from the rows the stage stored one
step earlier; a zero bound demands equality.  The cosines are the caller's: random fp16 in [-1, 1] with exact +-1 and 0 among them; the
packed weights come from real modules through cnerf_pack_field_chain16.

What the cases are for: H = 64 / 128 / 256 (NT 2 / 4 / 8: EPC 4 / 2 / 1, both cos prefetch distances); FiLM, feature + xyz, a pyramid
of five feature tiles in three levels, plain sine, one and two residual blocks (HAS_RES), no volume; 175 points per image (6 tiles: two
idle waves, a 15-row last tile) and 33 (a 1-row last tile); passes 0 and 1 storing gin, pass 2 adding to the volumes itself; an image
sub-range; FiLM frequencies 2^6 apart between the images of a chunk; rows spanning 2^24 inside every tile, and runs of power-of-two
copies of one point whose gin rows must be exact multiples; a dry run that samples every second group while one point of an unsampled
group carries 2^20 times the largest gradient (scales, the clamp report, +-65504), and the same input with every group sampled.

Buffers: every output sits between 64 KiB of a canary byte pattern that must be intact afterwards; with an image sub-range the g16 /
go16 / gin buffers hold only the chunk, the gradient volumes are the FULL tensors and the slots of the images outside the range (and
one slot behind the last) must keep their sentinel.

Measured worst |err| / bound over all cases (MI355X; each case prints its own):
    go16 0.99 (one fp16 rounding: attained)   the head's slab 0.76 - 0.89   lower slabs 0.09 - 0.34   gin 0.05 - 0.24   volumes 0.08 - 0.18
    0.84 - 0.99 in the slabs whose rows sit at the stored scale's floor 2^-25 / S, which is then the whole bound: the wide-range and copies
    cases, image 1 of the 2^6 case, the sampling case with every group sampled (the hot point sets the scales)
-- the float32 emulation of tests/test_chain16_cpu.py gives the same figures to the third digit.  No derived term had to be corrected on
the hardware, and no defect was found in bwd16.hip or the packing.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import chain16_common as K

pytestmark = pytest.mark.gpu

GUARD = 65536          # canary bytes on either side of every output
CANARY = 0xA5
SENT = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


class Guarded:
    """nbytes of device memory between two guards of canary bytes."""

    def __init__(self, nbytes, dev, fill=0xFF):
        self.n = nbytes
        self.raw = torch.full((nbytes + 2 * GUARD,), CANARY, dtype=torch.uint8, device=dev)
        self.raw[GUARD:GUARD + nbytes] = fill
        self.ptr = C.c_void_p(self.raw.data_ptr() + GUARD)

    def intact(self):
        return bool((self.raw[:GUARD] == CANARY).all()) and bool((self.raw[GUARD + self.n:] == CANARY).all())

    def view(self, dtype):
        return self.raw[GUARD:GUARD + self.n].view(dtype)


def run_case(dev, name):
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    lib = L.lib()
    cs, net = K.case(name)
    sn, H, NT, nslab = cs.sn, cs.sn.H, cs.sn.H // 32, cs.nslab
    net.to(dev)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    vols = [torch.zeros((cs.B, V, V, V, Cc), device=dev) for V, Cc in cs.levels]
    cfg = ops.make_cfg(net, cs.B, vols, cs.R, cs.Sr, precision="fp16x3", ray_start=0.25, ray_end=1.95, fov=49.13, hierarchical=True)
    packed16 = ops.pack_field_chain16(net, cfg)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    torch.manual_seed(3)
    cam = create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, cs.B), "y").to(dev).contiguous()
    u_strat = torch.rand((cs.B, cs.npi), device=dev)
    fine_z = (0.25 + 1.7 * torch.rand((cs.B, cs.npi), device=dev)).contiguous()
    up, saved, freq, pts = T(cs.upstream), T(cs.saved), T(cs.freq), T(cs.points)
    cos16 = torch.from_numpy(K.to_cos16(cs.cos, NT)).to(dev)
    tiles = cs.n_images * cs.tpi
    n = cs.n_images * cs.npi
    feat = cs.feature_tiles()
    own = cs.pss == 2 and bool(feat)                 # the chain adds to the volumes itself
    g16 = Guarded(nslab * tiles * NT * 2048, dev)
    go16 = Guarded(tiles * 2048, dev)
    scales = Guarded(8 * (nslab + 1), dev)
    gmax = Guarded(4 * (nslab + 2), dev)
    gin = Guarded(len(feat) * n * 128, dev) if feat and not own else None
    sat = Guarded(4, dev, fill=0)
    gvols, gvs = [], None
    if own:
        for (V, Cc), b in zip(cs.levels, cs.base):
            g = torch.full((cs.B + 1, V, V, V, Cc), SENT, device=dev)
            g[cs.image0:cs.image0 + cs.n_images] = T(b)
            gvols.append(g)
        gvs = ops.volumes_struct(gvols)
    rc = lib.cnerf_field_chain16(C.byref(cfg), cs.pss, cs.image0, cs.n_images, L.ptr(packed16), L.ptr(freq), L.ptr(cam), L.ptr(pts if cs.pss == 2 else u_strat),
                                 L.ptr(fine_z), L.ptr(up), L.ptr(saved), L.ptr(cos16), cs.group_step, g16.ptr, go16.ptr, scales.ptr, gmax.ptr,
                                 gin.ptr if gin else None, C.byref(gvs) if own else None, sat.ptr, stream)
    L.check(rc, "cnerf_field_chain16")
    torch.cuda.synchronize()
    for k, b in (("g16", g16), ("go16", go16), ("scales", scales), ("gmax", gmax), ("gin", gin), ("saturated", sat)):
        assert b is None or b.intact(), f"canary bytes around {k} were written"
    out = dict(go16=K.from_tb16(go16.view(torch.float16).cpu().numpy(), 1, tiles, 1)[0].astype(np.float32),
               g=K.from_tb16(g16.view(torch.float16).cpu().numpy(), nslab, tiles, NT).astype(np.float32),
               scales=scales.view(torch.float32).cpu().numpy(), gmax=gmax.view(torch.float32).cpu().numpy(),
               gin=gin.view(torch.float32).cpu().numpy().reshape(len(feat), n, 32) if gin else None, sat=int(sat.view(torch.int32).cpu()[0]))
    assert np.isfinite(out["g"]).all() and np.isfinite(out["go16"]).all(), "an output tile was left unwritten (0xFFFF is a NaN)"
    if own:
        outside = [b for b in range(cs.B + 1) if not cs.image0 <= b < cs.image0 + cs.n_images]
        for g in gvols:
            assert (g[outside] == SENT).all(), "a gradient volume slot outside the chunk was written"
        out["vols"] = [g[cs.image0:cs.image0 + cs.n_images].cpu().numpy() for g in gvols]
    r = K.check(cs, out, name + " ")
    assert not r.pop("broken")
    print(f"{name}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; saturated {out['sat']}")
    return cs, out


@pytest.mark.parametrize("name", [n for n in K.CASES if not n.startswith("sampling")])
def test_chain_rows_against_float64(dev, name):
    cs, out = run_case(dev, name)
    assert out["sat"] == 0


def test_sampled_dry_run_scales_and_the_clamp_report(dev):
    """Every second group sampled: the scales are the rule on the sampled rows, the hot point's tile is reported once per slab and its
    clamped elements are +-65504, every other row is inside its bound; with every group sampled the same input reports nothing."""
    cs, out = run_case(dev, "sampling_step2")
    assert out["sat"] == cs.nslab
    cs1, out1 = run_case(dev, "sampling_step1")
    assert out1["sat"] == 0 and np.array_equal(cs1.upstream, cs.upstream)
    assert (out1["scales"][0:2 * cs.nslab:2] < out["scales"][0:2 * cs.nslab:2]).all(), "the hot point lowers every slab's scale once it is sampled"
