"""cnerf_field_chain_pw16: the half-precision gradient chain of the per-point FiLM family (pwchain::chain_pre_kernel and
pwchain::pw_gm_kernel, csrc/chain_pw16.hip) with the launches the render runs around them -- head scale, chain_pre's dry run, the g_y
scales, the per-layer derivative maxima, chain_pre, pw_gm's dry run, g_mpre's scale, pw_gm -- ROW BY ROW against float64.

The formulas, the bounds and their derivations are in tests/chain_pw16_common.py; tests/test_chain_pw16_cpu.py shows that an honest
float32 emulation stays inside them and that each of fourteen named hazards exceeds one or breaks an equality.  Every element of go16,
of every g_y slab, of g_mpre and of the gradient volume is compared, each step from the rows the stage stored one step earlier; the 3 L
gradient slabs must equal fp16(gy16 d16 r_l) bit for bit; a zero bound demands equality.  The derivative rows, amax and m16 are the
caller's: random fp16 at realistic magnitudes with exact 0 and +-1 among them, padded rows filled with +-65504; the packed weights come
from real modules through cnerf_pack_field_chain16.

What the cases are for: H = 64 / 128 / 256 with the 8-layer TALLSIREN (NT 2 / 4 / 8: the prefetch slot wraps every tile at NT = 2, one
epilogue element rides per MFMA at NT = 8); test-local subclasses with 2 layers (two Y units, fewer than the ring's three slots) and
with 1 (no Y unit is ever requested); 175 points per image (6 tiles: two idle waves, a 15-row last tile) and 33 (a 1-row last tile);
passes 0, 1 and 2; an image sub-range of a B = 3 call; upstream rows spanning 2^20 inside every tile with hidden weights that put
consecutive layers' g_y 2^+-6 apart; runs of power-of-two copies of one point, whose g_y rows must be exact multiples; a non-zero base in
the gradient volume; dry runs that sample every second group while one point of an unsampled group carries 2^20 x the largest upstream
row (scales by the rule on the sampled rows, +-65504, `saturated`), the same input with every group sampled, and the intermediate case.

The intermediate case: a point of an unsampled group whose last-layer g_y is 15.9 x the sampled maximum's binade is stored finite and
unclamped by chain_pre; with a cos 15 pre row at the layer's largest value its mapping-product operands gy16 d To exceed 65504: +-inf in
about a fifth of the channels with both signs, all 256 g_m of the point NaN, fmaxf drops them, NaN goes into the voxels the point
reaches.  With the kernels as they were `saturated` stayed 0 (measured on an MI355X: 0, NaN in 4 voxels; the emulation:
test_chain_pw16_cpu.py::test_unreported_operand_range_gives_nan_with_saturated_zero): the documented contract did not hold.  Now
chain_pre_kernel counts every (tile, layer) with a point whose (max |g_y| S_y) amax To_l exceeds 65472: `saturated` is 1 here, every
other row and every voxel out of the hot point's reach is inside its bound.

Buffers: every output sits between 64 KiB of a canary byte pattern that must be intact afterwards and is pre-filled with 0xFF (an
unwritten tile is a NaN); the gradient volume is the FULL tensor plus one slot: the slots of the images outside the range and the one
behind the last must keep their sentinel.

One whole-chain check per width (not layer-local): the stage's volume gradient against the float64 chain run end to end from the same
inputs, relative L2 <= 2e-3, the gate of the render's backward tests.  Each case also prints the error of g_mpre relative to the POINT's
own magnitude for the points 2^-10 and 2^-20 below the largest (such points "contribute nothing").

Measured worst |err| / bound over all cases (MI355X; each case prints its own):
    go16 0.92 - 0.99 (one fp16 rounding: attained; 0 for the copies' 8-bit upstream)   gy16[L-1] 0.67 - 0.86   lower g_y slabs 0.13 - 0.35
    g_mpre 0.10 - 0.42, and 0.74 with the 2^20 outlier sampled (the rows sit at the stored scale's floor 2^-25 / S_mp)   volume 0.03 - 0.07
    whole chain end to end, relative L2: 8.4e-4 (H 64), 8.7e-4 (H 128), 8.6e-4 (H 256)
    g_mpre of a point 2^-10 / 2^-20 below the largest, error relative to its own magnitude: 1.4e-3 - 1.5e-3 / 1.3e-3 - 1.6e-3
    the 3 L slabs: bit-identical to fp16(gy16 d16 r_l) on every element of every case, subnormals included
-- the float32 emulation of tests/test_chain_pw16_cpu.py gives the same figures to the third digit.  Terms corrected on the hardware:
none.  One defect found: the unreported operand range of the intermediate case (above), fixed in chain_pre_kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_pw16_common as K

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


def launch(dev, name):
    """One call of the entry on the case's inputs: (case, the outputs check() reads)."""
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    lib = L.lib()
    cs, net = K.case(name)
    H, NT, Lc, V = cs.sn.H, cs.sn.H // 32, cs.L, cs.V
    net.to(dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cfg = ops.make_cfg(net, cs.B, [torch.zeros((cs.B, V, V, V, 32), device=dev)], cs.R, cs.Sr, precision="fp16x3", ray_start=0.25, ray_end=1.95,
                       fov=49.13, hierarchical=True)
    packed16 = ops.pack_field_chain16(net, cfg)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cam, u_strat, fine_z, up, saved, pts = T(cs.cams), T(cs.u_strat), T(cs.fine_z), T(cs.upstream), T(cs.saved), T(cs.points)
    cos16, amax, m16 = T(K.to_cos16(cs.cos, NT)), T(cs.amax), T(K.to_tb16(cs.m16, 8))
    tiles = cs.n_images * cs.tpi
    gy16 = Guarded(Lc * tiles * NT * 2048, dev)
    g16 = Guarded((3 * Lc * NT + 8) * tiles * 2048, dev)
    go16 = Guarded(tiles * 2048, dev)
    scales = Guarded(4 * (2 * (4 * Lc + 2) + 2 * Lc), dev)
    gmax = Guarded(4 * (5 * Lc + 2), dev)
    sat = Guarded(4, dev, fill=0)
    gvol = torch.full((cs.B + 1, V, V, V, 32), SENT, device=dev)
    gvol[cs.image0:cs.image0 + cs.n_images] = T(cs.base)
    gvs = ops.volumes_struct([gvol])
    rc = lib.cnerf_field_chain_pw16(C.byref(cfg), cs.pss, cs.image0, cs.n_images, L.ptr(packed16), L.ptr(cam), L.ptr(pts if cs.pss == 2 else u_strat),
                                    L.ptr(fine_z), L.ptr(up), L.ptr(saved), L.ptr(cos16), L.ptr(amax), L.ptr(m16), cs.group_step, gy16.ptr, g16.ptr,
                                    go16.ptr, scales.ptr, gmax.ptr, C.byref(gvs), sat.ptr, stream)
    L.check(rc, "cnerf_field_chain_pw16")
    torch.cuda.synchronize()
    for k, b in (("gy16", gy16), ("g16", g16), ("go16", go16), ("scales", scales), ("gmax", gmax), ("saturated", sat)):
        assert b.intact(), f"canary bytes around {k} were written"
    outside = [b for b in range(cs.B + 1) if not cs.image0 <= b < cs.image0 + cs.n_images]
    assert (gvol[outside] == SENT).all(), "a gradient volume slot outside the chunk was written"
    g = g16.view(torch.float16).cpu().numpy()
    n_slab = 3 * Lc * tiles * NT * 1024
    out = dict(go16=K.from_tb16(go16.view(torch.float16).cpu().numpy(), 1, tiles, 1)[0].astype(np.float32),
               gy=K.from_tb16(gy16.view(torch.float16).cpu().numpy(), Lc, tiles, NT).astype(np.float32),
               g=K.from_tb16(g[:n_slab], 3 * Lc, tiles, NT).astype(np.float32), gmp=K.from_tb16(g[n_slab:], 1, tiles, 8)[0].astype(np.float32),
               scales=scales.view(torch.float32).cpu().numpy(), gmax=gmax.view(torch.float32).cpu().numpy(),
               vols=gvol[cs.image0:cs.image0 + cs.n_images].cpu().numpy(), sat=int(sat.view(torch.int32).cpu()[0]))
    return cs, out


def run_case(dev, name):
    cs, out = launch(dev, name)
    hot = None if cs.hot is None else cs.hot[0] * cs.tpi * 32 + cs.hot[1]
    rest = np.arange(cs.rows) != hot
    assert all(np.isfinite(out[k]).all() for k in ("go16", "gy", "g")) and np.isfinite(out["gmp"][rest]).all(), \
        "an output tile was left unwritten (0xFFFF is a NaN), or a NaN was computed"
    r = K.check(cs, out, name + " ")
    assert not r.pop("broken")
    small = K.small_point_report(cs, np.where(rest[:, None], out["gmp"], 0.0), float(out["scales"][2 * 3 * cs.L]))
    print(f"{name}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; saturated {out['sat']}; g_mpre error relative to the "
          f"point's own magnitude, points 2^-10 below the largest: {small[10]:.3g}, 2^-20 below: {small[20]:.3g}")
    return cs, out


@pytest.mark.parametrize("name", [n for n in K.CASES if "step" not in n])
def test_chain_rows_against_float64(dev, name):
    cs, out = run_case(dev, name)
    assert out["sat"] == 0
    if name in K.WHOLE_CHAIN:
        rel = K.whole_chain_rel_l2(cs, out["vols"])
        print(f"{name}: volume gradient against the float64 chain end to end, relative L2 {rel:.3g}")
        assert rel <= 2e-3


def test_sampled_dry_runs_scales_and_the_clamp_report(dev):
    """Every second group sampled: the scales are the rule on the sampled rows, the hot point's tile is reported once per layer, its
    clamped g_y elements are +-65504, every other row and every voxel out of the hot point's reach is
    inside its bound; with every group sampled the same input reports nothing."""
    cs, out = run_case(dev, "sampling_step2")
    assert out["sat"] == cs.L
    cs1, out1 = run_case(dev, "sampling_step1")
    assert out1["sat"] == 0 and np.array_equal(cs1.upstream, cs.upstream)
    sy = lambda o: o["scales"][2 * (3 * cs.L + 2)::2][:cs.L]
    assert (sy(out1) < sy(out)).all(), "the hot point lowers every layer's g_y scale once it is sampled"


def test_operands_beyond_fp16_are_reported(dev):
    """The intermediate case: g_y stored unclamped, operands gy16 d To beyond 65504.  The documented contract: either every output is
    finite and in bound, or saturated > 0.  chain_pre counts the (tile, layer); check() holds every row and voxel out of the point's reach."""
    cs, out = run_case(dev, "intermediate_step2")
    hot = cs.hot[0] * cs.tpi * 32 + cs.hot[1]
    assert out["sat"] == 1 and 32000 < np.abs(out["gy"][cs.L - 1][hot]).max() < 65504 / 2
