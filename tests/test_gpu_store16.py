"""The fp16 activation rows of the storing forward (csrc/field_h3.hip, field_h3_kernel<NT, STORE_TB16, HAS_RES, WF>), ROW BY ROW against
float64, through the two launches that store them in production:

    kept      cnerf_render_forward with aux->act16 set (WF = 1 FiLM networks, WF = 2 plain-sine and residual ones: per-image folded weights);
    re-run    cnerf_field_store16, the launch chunk16 of cnerf_render_backward runs (WF = 0), on an image sub-range of passes 0, 1 and 2.

The conditions, their derivations and the layouts are in tests/store16_common.py: (a) equalities -- layout, input tiles bit for bit, padded
rows, untouched memory, rgb_sigma --, (b) sin^2 + cos^2, (c) every slab from the launch's own previous slab, (d) the share of sines beyond
one fp16 ulp of the float64 network against the same share of the reference's own fp32 evaluation.  tests/test_store16_cpu.py shows that
an honest float32 emulation passes them and that each named hazard fails one.

Shapes: H = 64 / 128 / 256 (NT 2 / 4 / 8; the KCH < 16 tail exists at 64 / 128); every family at H = 64, three of them at 128 and 256;
B = 3 images with distinct volumes, latents and FiLM vectors; 5 x 5 rays x 14 samples = 350 points per image (10 full tiles, a 30-row
tile, one idle wave), both passes, forced fine_z; the stage on images 1..2 and on image 2 alone; pass 2 with 33 points per image (a 1-row
last tile, three idle waves) and with 128 (no idle wave).  Every buffer lies between guards and starts as an fp16 NaN canary.  One more
stage call, SHORTSIREN_FG at H = 64 on pass 2: images 0..1 with so many points that the tile groups are about 2.5 x the CU count and no
multiple of 8 -- every block takes its second and third trip through the tile loop, and every element is checked as above.

Measured on an MI355X (each launch prints its own line).  Every equality holds on every launch, the input tiles of all levels included.
Worst |err| / bound over a network's eight launches, and for (d) the launch and slab with the kernel's largest share beyond one fp16 ulp
as (kernel share, the reference's own fp32 share), kept path | stage path; the largest deviation in ulps, kernel / reference:
    network               (b) pair       (c) sin        (c) cos        (d) kept            (d) stage           ulps
    SHORTSIREN_FG 64      0.693 - 0.702  0.469 - 0.491  0.475 - 0.485  (0.0048, 0.0022)    (0.0052, 0.0038)    330 / 95
    SHORTSIREN_F 64       0.508 - 0.513  0.729 - 0.754  0.501 - 0.502  (0.0000, 0.0000)    (0.0000, 0.0000)    1 / 1
    SHORTSIREN_FRes 64    0.539 - 0.545  0.698 - 0.791  0.513 - 0.523  (0.0001, 0.0000)    (0.0002, 0.0000)    2 / 1
    TALLSIREN_dRes 64     0.541 - 0.552  0.800 - 0.885  0.534 - 0.552  (0.0002, 0.0000)    (0.0005, 0.0000)    2 / 1
    TALLSIREN_dgx 64      0.699 - 0.702  0.477 - 0.521  0.473 - 0.510  (0.0018, 0.0009)    (0.0014, 0.0011)    85 / 52
    SHORTSIREN_FG_Pyrmd   0.693 - 0.702  0.525 - 0.648  0.484 - 0.794  (0.0040, 0.0019)    (0.0031, 0.0031)    200 / 118
    SHORTSIREN 64         0.688 - 0.702  0.779 - 0.890  0.806 - 0.904  (0.0009, 0.0005)    (0.0009, 0.0006)    62 / 39
    SingleSIREN_dg 64     0.686 - 0.702  0.473 - 0.511  0.462 - 0.496  (0.0003, 0.0001)    (0.0003, 0.0001)    16 / 8
    TALLSIREN_FG 64       0.699 - 0.702  0.467 - 0.513  0.495 - 0.525  (0.0014, 0.0006)    (0.0012, 0.0006)    96 / 61
    SHORTSIREN_FG 128     0.697 - 0.702  0.475 - 0.567  0.477 - 0.555  (0.0051, 0.0026)    (0.0036, 0.0022)    196 / 100
    SHORTSIREN_FRes 128   0.512 - 0.541  0.707 - 0.859  0.504 - 0.529  (0.0000, 0.0000)    (0.0001, 0.0000)    2 / 1
    TALLSIREN_dgx 128     0.702 - 0.702  0.582 - 0.699  0.502 - 0.554  (0.0016, 0.0011)    (0.0018, 0.0012)    86 / 105
    SHORTSIREN_FG 256     0.692 - 0.702  0.481 - 0.747  0.471 - 0.568  (0.0048, 0.0031)    (0.0041, 0.0036)    621 / 401
    SHORTSIREN_FRes 256   0.532 - 0.550  0.730 - 0.781  0.509 - 0.530  (0.0000, 0.0000)    (0.0001, 0.0000)    2 / 1
    TALLSIREN_dgx 256     0.702 - 0.702  0.527 - 0.619  0.481 - 0.516  (0.0018, 0.0011)    (0.0013, 0.0013)    239 / 113
-- the float32 emulation of tests/test_store16_cpu.py gives pair 0.50 - 0.70 and sin / cos 0.44 - 0.91.  The pair identity tops out at
0.702 as derived; (c) is widest where layer 0 reads the position itself (its fp16 rounding is the bound).  The narrowest (d) margin is
TALLSIREN_dRes' 33-point stage call: 0.0005 of the elements against the allowed 0 + 1e-3.  Terms corrected on the hardware: none.  No
defect was found in field_h3.hip, the fold kernels or the host layer.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import store16_common as K

pytestmark = pytest.mark.gpu

GUARD = 65536          # canary bytes on either side of every buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


class Guarded:
    """n fp16 elements (or fp32 with words=True) of device memory between two guards; the interior starts as the canary NaN."""

    def __init__(self, n, dev, words=False):
        self.nbytes = n * (4 if words else 2)
        self.raw = torch.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        inner = self.raw[GUARD:GUARD + self.nbytes]
        if words:
            inner.view(torch.float32).fill_(float("nan"))
        else:
            inner.view(torch.int16).fill_(K.CANARY16)
        self.t = inner.view(torch.float32 if words else torch.float16)
        self.ptr = C.c_void_p(self.raw.data_ptr() + GUARD)

    def intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def numpy(self):
        return self.t.cpu().numpy()


class Net:
    """One network on the device with its inputs, packed weights and camera."""

    def __init__(self, dev, variant, H, hot_feature=None):
        import cnerf_amd
        from cnerf_amd import ops
        from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix
        self.ops, self.L, self.dev = ops, cnerf_amd._lib, dev
        self.cs, self.net = K.make_case(variant, H, hot_feature=hot_feature)
        self.net.to(dev)
        self.net.precision = "fp16x3"
        T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.vols = [T(v) for v in self.cs.vols]
        self.freq, self.phase = T(self.cs.freq), T(self.cs.phase)
        g = np.random.default_rng(5)            # camera origins on shells r in [0.7, 1.5], away from the poles: the same on every run
        B = self.cs.B
        theta, phi, r = np.clip(np.arccos(1 - g.random(B)), 0.2, np.pi - 0.2), 2 * np.pi * g.random(B), 0.7 + 0.8 * g.random(B)
        origin = np.stack([r * np.sin(theta) * np.cos(phi), r * np.cos(theta), r * np.sin(theta) * np.sin(phi)], axis=1)
        self.cam = create_cam2world_matrix(torch.from_numpy(origin.astype(np.float32)), "y").to(dev).contiguous()
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def cfg(self, R, S_):
        return self.ops.make_cfg(self.net, self.cs.B, self.vols, R, S_, precision="fp16x3", ray_start=0.25, ray_end=1.95, fov=49.13, hierarchical=True)

    def buffers(self, tiles):
        cs = self.cs
        NT, n_in = cs.sn.H // 32, len(cs.tiles_in)
        return Guarded(tiles * n_in * 1024, self.dev), Guarded(cs.nslab * tiles * NT * 1024, self.dev), Guarded(cs.nslab * tiles * NT * 1024, self.dev)

    def gather(self, points):
        """fp32 lookups (B, npi, 32) per feature tile at the FULL points (B, npi, 3): cnerf_gather_features on the tile's 32 channels."""
        pts = torch.from_numpy(points).to(self.dev)
        return [self.ops.gather_features(self.net, self.vols[lvl][..., cc:cc + 32].contiguous(), pts).cpu().numpy() for lvl, cc in self.cs.tiles_in if lvl >= 0]

    def field_forward(self, cfg, points):
        """rgb_sigma (B, npi, 4) of the non-storing fp16x3 kernel at the FULL points."""
        ops, L = self.ops, self.L
        pts = torch.from_numpy(points).to(self.dev)
        out = torch.empty(points.shape[:2] + (4,), device=self.dev)
        L.check(L.lib().cnerf_field_forward(C.byref(cfg), C.byref(ops.volumes_struct(self.vols)), L.ptr(ops.pack_field(self.net, cfg)), L.ptr(self.freq),
                                            L.ptr(self.phase), L.ptr(pts), points.shape[1], L.ptr(out), self.stream), "cnerf_field_forward")
        return out.cpu().numpy()

    def judge(self, what, la, bufs, gather_full, ref=None, inputs_only=False):
        """Guards, decode and every check of store16_common for one launch; prints the launch's line."""
        cs = self.cs
        torch.cuda.synchronize()
        for k, b in zip(("feat", "h", "c"), bufs):
            assert b.intact(), f"{what}: guard bytes around {k} were written"
        out = K.decode(cs, la, dict(zip(("feat", "h", "c"), (b.numpy() for b in bufs))))
        out["gather"] = [g[la.image0:la.image0 + la.n_images].reshape(-1, 32) for g in gather_full]
        ref = ref if ref is not None or inputs_only else K.reference(cs, la)
        r = K.check(cs, la, out, ref=ref, tag=f"{cs.variant} H={cs.sn.H} {what} ", inputs_only=inputs_only)
        assert not r.pop("broken")
        if inputs_only:
            return out, r
        e2e = r.pop("e2e")
        worst = {p: max(v for k, v in r.items() if k.startswith(p)) for p in ("pair", "sin", "cos")}
        m, e = max(enumerate(e2e), key=lambda me: me[1][0])
        print(f"{cs.variant} H={cs.sn.H} {what}: worst |err| / bound pair {worst['pair']:.3f} sin {worst['sin']:.3f} cos {worst['cos']:.3f}; (d) slab {m} share "
              f"{e[0]:.4f} ({e[1]:.0f} ulps), reference's fp32 {e[2]:.4f} ({e[3]:.0f} ulps)")
        if la.n_images > 1:
            far = K.far_from_other_image(cs, la, out, ref[0])
            assert far > 0.2, f"{what}: the first image's rows are {far:.3g} of their size from the second image's expectation"
        return out, r

    def stage(self, cfg, pss, image0, n_images, points_full, gather_full, what):
        """cnerf_field_store16 on a sub-range; returns what judge() returns.  points_full (B, npi, 3): the pass's positions."""
        ops, L = self.ops, self.L
        la = K.Launch(image0, n_images, points_full[image0:image0 + n_images])
        bufs = self.buffers(la.tiles)
        rs = Guarded(n_images * la.npi * 4, self.dev, words=True)
        pts = torch.from_numpy(points_full).to(self.dev)
        u_strat = self.u_strat if pss != 2 else pts
        L.check(L.lib().cnerf_field_store16(C.byref(cfg), pss, image0, n_images, C.byref(ops.volumes_struct(self.vols)) if self.vols else None,
                                            L.ptr(ops.pack_field(self.net, cfg)), L.ptr(self.freq), L.ptr(self.phase), L.ptr(self.cam), L.ptr(u_strat),
                                            L.ptr(self.fine_z) if pss == 1 else None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, rs.ptr, self.stream), "cnerf_field_store16")
        out = self.judge(what, la, bufs, gather_full)
        assert rs.intact(), f"{what}: guard bytes around rgb_sigma were written"
        want = self.field_forward(cfg, points_full)[image0:image0 + n_images].reshape(-1, 4)
        assert np.array_equal(rs.numpy().reshape(-1, 4), want), f"{what}: rgb_sigma differs from the non-storing fp16x3 kernel's"
        return out

    def render(self, act16):
        ops = self.ops
        R, S_ = K.R_RENDER, K.S_RENDER
        return ops.render_forward(self.net, self.vols, self.freq, self.phase, self.cam, R, 49.13, 0.25, 1.95, S_, True, "relu", 0.0,
                                  rng=dict(u_strat=self.u_strat, u_fine=self.u_fine, fine_z=self.fine_z), want_aux=True, fvol_is_channel_last=True, act16=act16)

    def draws(self):
        B, P, S_ = self.cs.B, K.R_RENDER ** 2, K.S_RENDER
        g = torch.Generator().manual_seed(17)
        self.u_strat, self.u_fine = (torch.rand((B, P, S_), generator=g).to(self.dev) for _ in range(2))
        self.fine_z = (0.25 + 1.7 * torch.rand((B, P, S_), generator=g)).to(self.dev).contiguous()


@pytest.mark.parametrize("variant,H", [("SHORTSIREN_FG", 64)])
def test_stored_rows_when_every_block_takes_a_second_and_third_trip(dev, variant, H):
    """The stage alone, pass 2, images 0..1, on the long shape of tests/test_gpu_store_pw16.py (store_pw16_common.long_shape: 2 ceil(tiles
    per image / 4) tile groups are about 2.5 x the CU count and no multiple of 8, the last tile ragged), through stage() and with it
    every check of the test below, (d) included.  About 41 k points per image on 256 CUs: the test takes 2.6 s there, the float64 and
    float32 reference networks of eight 64-wide layers included."""
    import store_pw16_common
    nt = Net(dev, variant, H)
    R, S_ = store_pw16_common.long_shape(torch.cuda.get_device_properties(dev).multi_processor_count)
    points = K.random_points(nt.cs, R * R * S_, 23)
    nt.stage(nt.cfg(R, S_), 2, 0, 2, points, nt.gather(points), f"stage points {R * R * S_}")


@pytest.mark.parametrize("variant,H", K.NETS)
def test_stored_rows_against_float64(dev, variant, H):
    nt = Net(dev, variant, H)
    cs = nt.cs
    B, npi = cs.B, K.R_RENDER ** 2 * K.S_RENDER
    tpi = (npi + 31) // 32
    nt.draws()
    # kept path: the render with and without act16
    px0, dp0, aux0 = nt.render(None)
    kept = [nt.buffers(B * tpi) for _ in range(2)]
    px1, dp1, aux1 = nt.render([tuple(b.t for b in bufs) for bufs in kept])
    torch.cuda.synchronize()
    assert torch.equal(px0, px1) and torch.equal(dp0, dp1), "keeping the activations changed the image"
    for k in ("coarse_rgb_sigma", "fine_rgb_sigma", "coarse_points", "fine_points"):
        assert torch.equal(aux0[k], aux1[k]), f"keeping the activations changed {k}"
    cfg = nt.cfg(K.R_RENDER, K.S_RENDER)
    for pss, name in enumerate(("coarse", "fine")):
        points = aux0[name + "_points"].reshape(B, npi, 3).cpu().numpy()
        assert np.isfinite(points).all()
        gather = nt.gather(points)
        la = K.Launch(0, B, points)
        ref = K.reference(cs, la)
        nt.judge(f"kept {name}", la, kept[pss], gather, ref=ref)
        # the re-run on images 1..2 and on image 2 alone
        nt.stage(cfg, pss, 1, 2, points, gather, f"stage {name} images 1..2")
        nt.stage(cfg, pss, 2, 1, points, gather, f"stage {name} image 2")
    # pass 2: 33 points per image (a 1-row last tile, three idle waves), 128 (no idle wave)
    for R, S_, image0, n_images in ((1, 33, 1, 2), (2, 32, 0, 3)):
        points = K.random_points(cs, R * R * S_, 23)
        nt.stage(nt.cfg(R, S_), 2, image0, n_images, points, nt.gather(points), f"stage points {R * R * S_}")


def test_feature_of_7e4_is_stored_as_65504(dev):
    nt = Net(dev, "SHORTSIREN_FG", 64, hot_feature=7e4)
    nt.draws()
    points = K.random_points(nt.cs, 33, 23)
    gather = nt.gather(points)
    assert (gather[0][..., 5] > 65504.0).all()
    la = K.Launch(0, 3, points)
    bufs = nt.buffers(la.tiles)
    rs = Guarded(la.n_images * 33 * 4, dev, words=True)
    ops, L = nt.ops, nt.L
    cfg = nt.cfg(1, 33)
    L.check(L.lib().cnerf_field_store16(C.byref(cfg), 2, 0, 3, C.byref(ops.volumes_struct(nt.vols)), L.ptr(ops.pack_field(nt.net, cfg)), L.ptr(nt.freq),
                                        L.ptr(nt.phase), None, L.ptr(torch.from_numpy(points).to(dev)), None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, rs.ptr,
                                        nt.stream), "cnerf_field_store16")
    out, _ = nt.judge("hot feature", la, bufs, gather, inputs_only=True)
    assert (out["feat"][:, 5] == 65504.0).all() and np.isfinite(out["feat"]).all()
