"""Depth maps <-> clouds on the GPU: cnerf_backproject and cnerf_splat_points through ops (and once through ctypes alone) against their
NumPy statements (tests/reproject_common.py), bit for bit on every output; the round trip on the device; views.render_pcl on a small
generator; the trainer's depth term.  Every case is a few thousand pixels or points, but for the two that outgrow a round of the scan
(98,304 pixels) and the splat's launch grid (90,000 points into 540,000 pixels)."""
import ctypes as C

import numpy as np
import pytest
import torch

import reproject_common as RC

pytestmark = pytest.mark.gpu

F = np.float32
Z_MIN, Z_MAX = 0.25, 1.95
FOCAL = RC.focal32()
FOV = 49.134342641202636


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def host(t):
    return None if t is None else t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# back-projection
# ---------------------------------------------------------------------------------------------------------------------
def bp_case(V, R, seed):
    """View 0: depths inside, below, above, exactly z_min, exactly z_max, NaN, +-inf, 0.  View 1: no valid pixel.  The last view: every
    pixel valid.  Views between them (V = 6) as view 0.  V = 2 has no view without a valid pixel: the first wave of view 0 (64 pixels)
    is invalid throughout instead, and its second wave valid throughout."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 1.8, (V, R, R)).astype(F)
    kind = rng.integers(0, 16, (V, R, R))
    for k, val in enumerate((0.1, 2.5, Z_MIN, Z_MAX, np.nan, np.inf, -np.inf, 0.0)):
        depth[kind == k] = val
    depth[1] = rng.choice(np.asarray([0.0, 0.1, Z_MIN, Z_MAX, 2.5, np.nan, np.inf], F), (R, R))
    depth[V - 1] = rng.uniform(0.26, 1.94, (R, R)).astype(F)
    if V == 2:
        depth[0].reshape(-1)[:64] = 0.0
        depth[0].reshape(-1)[64:128] = rng.uniform(0.26, 1.94, 64).astype(F)
    colors = rng.uniform(-1, 1, (V, 3, R, R)).astype(F)
    mask = rng.choice(np.asarray([0.0, 1e-4, 2e-4, 1.0, np.nan], F), (V, R, R))
    return depth, RC.cameras(V, seed + 100), colors, mask


def gpu_backproject(dev, depth, cams, **kw):
    from cnerf_amd import ops
    for k in ("colors", "mask"):
        if kw.get(k) is not None:
            kw[k] = on(dev, kw[k], F)
    if "color_layout" in kw:
        kw["color_layout"] = {0: "chw", 1: "hwc"}[kw["color_layout"]]
    out = ops.backproject(on(dev, depth, F), on(dev, cams, F), float(FOCAL), Z_MIN, Z_MAX, want_pixel=True, want_rank=True, **kw)
    assert out[0].dtype == torch.float32 and all(t.dtype == torch.int32 for t in out[1:]) and not out[0].requires_grad
    return tuple(host(t) for t in out)


def assert_cloud(got, want, what):
    assert RC.same_bits(got[0], want[0]), what
    for g, w, name in zip(got[1:], want[1:], ("counts", "pixel", "rank")):
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("V,R", [(3, 5), (2, 17), (3, 33), (6, 128)])
def test_backproject_equals_the_statement(dev, V, R):
    """R = 5: a view is smaller than a wave.  V = 2 at R = 17: 289 pixels per view, so a view's second chunk holds 33 of them -- a full
    wave is absent, the last wave has one lane -- and the boundary between the views falls inside the flat scan.  R = 33: 1,089 pixels
    per view, 3,267 in all, a multiple of neither 64 nor 256.  V = 6 at R = 128: 98,304 pixels = 384 chunks of 256 pixels (BP_CHUNK),
    more than the 256 counts one round of the scan takes."""
    depth, cams, colors, mask = bp_case(V, R, 7 * V + R)
    hwc = np.ascontiguousarray(colors.transpose(0, 2, 3, 1))
    seen = 0
    for what, kw in (("no colours", {}), ("chw, mask", dict(colors=colors, color_layout=0, mask=mask, mask_min=1e-4)),
                     ("hwc", dict(colors=hwc, color_layout=1)), ("chw, 0.5 / 0.5", dict(colors=colors, color_layout=0, color_scale=0.5, color_offset=0.5)),
                     ("mask alone, at 0", dict(mask=mask))):
        want = RC.backproject32(depth, cams, FOCAL, Z_MIN, Z_MAX, **kw)
        got = gpu_backproject(dev, depth, cams, **kw)
        assert_cloud(got, want, what)
        counts = want[1]
        assert counts[0] > 0 and (V == 2 or counts[1] == 0) and counts[V - 1] == (R * R if "mask" not in kw else counts[V - 1]) and got[0].shape[1] == (6 if "colors" in kw else 3)
        seen += len(want[0])
    assert seen > 0
    if R == 128:
        assert V * -(-R * R // 256) > 256
    hw = RC.backproject32(depth, cams, FOCAL, Z_MIN, Z_MAX, colors=hwc, color_layout=1)
    ch = RC.backproject32(depth, cams, FOCAL, Z_MIN, Z_MAX, colors=colors, color_layout=0)
    assert RC.same_bits(hw[0], ch[0])                                 # the two layouts hold the same colours


def test_backproject_through_ctypes_alone(dev):
    """A caller-made workspace filled with garbage, outputs pre-filled with a sentinel; then with every optional output NULL."""
    from cnerf_amd import ops, _lib as L
    lib = L.lib()
    V, R = 3, 33
    depth, cams, colors, mask = bp_case(V, R, 5)
    want = RC.backproject32(depth, cams, FOCAL, Z_MIN, Z_MAX, colors=colors, mask=mask, mask_min=1e-4)
    n = len(want[0])
    nb = C.c_size_t(0)
    L.check(lib.cnerf_backproject_bytes(V, R, C.byref(nb)), "bytes")
    d, cm, co, mk = on(dev, depth, F), on(dev, cams.reshape(V, 16), F), on(dev, colors, F), on(dev, mask, F)
    for optional in (True, False):
        ws = torch.full((nb.value,), 0xA5, dtype=torch.uint8, device=dev)
        pts = torch.full((V * R * R, 6), 12345.0, dtype=torch.float32, device=dev)
        counts = torch.full((V,), -77, dtype=torch.int32, device=dev) if optional else None
        pixel = torch.full((V * R * R,), -77, dtype=torch.int32, device=dev) if optional else None
        rank = torch.full((V, R, R), -77, dtype=torch.int32, device=dev) if optional else None
        L.check(lib.cnerf_backproject(V, R, L.ptr(d), L.ptr(co), 0, L.ptr(mk), 1e-4, L.ptr(cm), float(FOCAL), Z_MIN, Z_MAX, 1.0, 0.0, L.ptr(pts),
                                      L.ptr(counts), L.ptr(pixel), L.ptr(rank), L.ptr(ws), ops._stream()), "backproject")
        assert RC.same_bits(host(pts)[:n], want[0]) and (host(pts)[n:] == 12345.0).all()          # the rows behind the cloud are not written
        if optional:
            assert np.array_equal(host(counts), want[1]) and np.array_equal(host(pixel)[:n], want[2]) and np.array_equal(host(rank), want[3])
            assert (host(pixel)[n:] == -77).all()


def test_backproject_refuses(dev):
    from cnerf_amd import ops
    from cnerf_amd import _lib
    CnerfError = _lib.CnerfError
    depth, cams, colors, mask = bp_case(3, 5, 1)
    d, c = on(dev, depth, F), on(dev, cams, F)
    with pytest.raises(CnerfError):
        ops.backproject(d.cpu(), c.cpu(), 2.18, Z_MIN, Z_MAX)         # no CPU fallback
    for kw in (dict(colors=on(dev, colors, F), color_layout="hwc"), dict(color_layout="nchw"), dict(mask=on(dev, mask[:2], F))):
        with pytest.raises(CnerfError):
            ops.backproject(d, c, 2.18, Z_MIN, Z_MAX, **kw)
    for args in ((d, c[:2], 2.18, Z_MIN, Z_MAX), (d, c, 0.0, Z_MIN, Z_MAX), (d, c, 2.18, Z_MAX, Z_MIN), (d[:, :4], c, 2.18, Z_MIN, Z_MAX)):
        with pytest.raises(CnerfError):
            ops.backproject(*args)


# ---------------------------------------------------------------------------------------------------------------------
# splat
# ---------------------------------------------------------------------------------------------------------------------
def gpu_splat(dev, pts, cams, R, radius, lengths=None, **kw):
    from cnerf_amd import ops
    want_pixels = pts.shape[-1] >= 6
    out = ops.splat_points(on(dev, pts, F), on(dev, cams, F), R, float(FOCAL), Z_MIN, Z_MAX, radius=radius, lengths=on(dev, lengths, np.int32),
                           want_pixels=want_pixels, **kw)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and (out[2] is None) == (not want_pixels)
    return tuple(host(t) for t in out)


def assert_picture(got, want, what):
    assert RC.same_bits(got[0], want[0]), (what, "depth")
    assert np.array_equal(got[1], want[1]), (what, "index")
    assert (got[2] is None and want[2] is None) or RC.same_bits(got[2], want[2]), (what, "pixels")


def splat_cloud(B, n, V, R, seed, stride=6):
    """Random coloured points around the origin; from row 8 on, where n allows, per image: a point behind camera 0, one beyond z_max, one with
    a NaN coordinate, one far outside the image, and twenty-four whose footprints are cut by each border and each corner of camera 0's image
    (projections 0.2 px inside and 0.7 px outside the border pixels)."""
    rng = np.random.default_rng(seed)
    cams = RC.cameras(B * V, seed + 1).reshape(B, V, 4, 4)
    pts = np.concatenate([rng.uniform(-0.55, 0.55, (B, n, 3)), rng.uniform(0, 1, (B, n, stride - 3))], 2).astype(F)
    for b in range(B):
        M = cams[b, 0]
        special = [RC.lift64(M, R / 2, R / 2, -0.5, R, FOCAL), RC.lift64(M, R / 2, R / 2, 2.5, R, FOCAL), np.asarray([np.nan, 0.1, 0.2], F),
                   RC.lift64(M, 40.0 * R, -30.0 * R, 1.0, R, FOCAL)]
        edge = (-0.7, 0.2, R / 2, R - 1.2, R - 0.3)
        special += [RC.lift64(M, r, c, 0.8 + 0.01 * k, R, FOCAL) for k, (r, c) in enumerate((r, c) for r in edge for c in edge) if (r, c) != (R / 2, R / 2)]
        for k, p in enumerate(special):
            if 8 + k < n:
                pts[b, 8 + k, :3] = p
    return pts, cams


@pytest.mark.parametrize("R", [7, 32])
@pytest.mark.parametrize("radius", [0, 1, 3])
def test_splat_equals_the_statement(dev, R, radius):
    B, V = 2, 3
    for n, lengths in ((1, None), (65, None), (5000, (5000, 1234))):
        pts, cams = splat_cloud(B, n, V, R, 3 * n + R)
        want = RC.splat32(pts, cams, R, FOCAL, Z_MIN, Z_MAX, radius, lengths)
        got = gpu_splat(dev, pts, cams, R, radius, lengths)
        assert_picture(got, want, (n, "against the statement"))
        assert_picture(gpu_splat(dev, pts, cams, R, radius, lengths), got, (n, "two runs"))
        if n >= 65:
            hit = want[1] >= 0
            assert hit.any() and (want[0][~hit] == 0).all() and (want[2][~hit] == 1).all()
            assert hit[:, 0, 0, :].any() and hit[:, 0, -1, :].any() and hit[:, 0, :, 0].any() and hit[:, 0, :, -1].any()      # the borders were reached
        if lengths is not None:
            assert want[1][1].max() < 1234 <= want[1][0].max()


def test_splat_contention_and_ties(dev):
    """2,000 points on one ray of camera 0 with distinct depths, shuffled: they contend on one pixel and the nearest wins.  Then the
    same point stored at several indices: the lowest index wins.  Both at radius 0 and 1."""
    R, B, V = 32, 2, 3
    rng = np.random.default_rng(9)
    cams = RC.cameras(B * V, 10).reshape(B, V, 4, 4)
    zs = rng.permutation(np.linspace(0.4, 1.8, 2000))
    ray = np.stack([np.stack([RC.lift64(cams[b, 0], 11, 20, z, R, FOCAL) for z in zs]) for b in range(B)])
    pts = np.concatenate([ray, rng.uniform(0, 1, (B, 2000, 3)).astype(F)], 2)
    dup = np.concatenate([rng.uniform(-0.4, 0.4, (B, 50, 3)), rng.uniform(0, 1, (B, 50, 3))], 2).astype(F)
    dup = np.tile(dup, (1, 4, 1))                                     # every point at indices k, k + 50, k + 100, k + 150, other colours
    dup[..., 3:] = rng.uniform(0, 1, dup[..., 3:].shape)
    for radius in (0, 1):
        want = RC.splat32(pts, cams, R, FOCAL, Z_MIN, Z_MAX, radius)
        assert_picture(gpu_splat(dev, pts, cams, R, radius), want, "one ray")
        z32 = RC.project32(pts[0, :, :3], cams[0, 0], FOCAL, R)[0]
        assert want[1][0, 0, 11, 20] == int(np.argmin(z32)) and want[0][0, 0, 11, 20] == z32.min()
        want = RC.splat32(dup, cams, R, FOCAL, Z_MIN, Z_MAX, radius)
        assert_picture(gpu_splat(dev, dup, cams, R, radius), want, "duplicates")
        assert (want[1] < 50).all() and (want[1] >= 0).sum() > 50


def test_splat_strides_and_optional_outputs(dev):
    from cnerf_amd import ops
    from cnerf_amd import _lib
    CnerfError = _lib.CnerfError
    R, B, V = 32, 2, 3
    pts, cams = splat_cloud(B, 700, V, R, 21, stride=8)
    want = RC.splat32(pts, cams, R, FOCAL, Z_MIN, Z_MAX, 1, background=(0.25, 0.5, 0.75))
    assert_picture(gpu_splat(dev, pts, cams, R, 1, background=(0.25, 0.5, 0.75)), want, "stride 8")
    xyz = np.ascontiguousarray(pts[..., :3])
    got = gpu_splat(dev, xyz, cams, R, 1)
    assert got[2] is None and RC.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1])
    p, c = on(dev, xyz, F), on(dev, cams, F)
    with pytest.raises(CnerfError):
        ops.splat_points(p, c, R, float(FOCAL), Z_MIN, Z_MAX, want_pixels=True)       # colours need stride >= 6
    with pytest.raises(CnerfError):
        ops.splat_points(p.cpu(), c.cpu(), R, float(FOCAL), Z_MIN, Z_MAX, want_pixels=False)
    for kw in (dict(radius=9), dict(radius=-1), dict(lengths=torch.tensor([1], device=dev))):
        with pytest.raises(CnerfError):
            ops.splat_points(p, c, R, float(FOCAL), Z_MIN, Z_MAX, want_pixels=False, **kw)
    with pytest.raises(CnerfError):
        ops.splat_points(p, c[:1], R, float(FOCAL), Z_MIN, Z_MAX, want_pixels=False)


def test_splat_beyond_the_launch_grid(dev):
    """Both splat kernels stride over their work with at most 2,048 blocks of 256 lanes (SPLAT_MAX_GRID of csrc/reproject.hip): 2 x 3 views
    x 90,000 points are 2,112 blocks' worth, 2 x 3 x 300 x 300 pixels 2,110."""
    B, V, R, n = 2, 3, 300, 90000
    assert B * V * -(-n // 256) > 2048 and -(-B * V * R * R // 256) > 2048
    pts, cams = splat_cloud(B, n, V, R, 33)
    want = RC.splat32(pts, cams, R, FOCAL, Z_MIN, Z_MAX, 0, (n, n - 3))
    assert_picture(gpu_splat(dev, pts, cams, R, 0, (n, n - 3)), want, "beyond the grid")
    assert (want[1] >= 0).mean() > 0.2 and want[1].max() > n - 1000


# ---------------------------------------------------------------------------------------------------------------------
# both together
# ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_on_the_device(dev):
    """ops.backproject then ops.splat_points at radius 0.  A view's own points into its own camera: index == rank and depth within
    16 2^-24 (|p|_1 + |t|_1) of the depth map (the count is in tests/test_reproject_cpu.py).  The fused cloud into each of the V
    cameras: the statement's picture, bit for bit."""
    from cnerf_amd import ops
    V, R = 3, 33
    depth, cams, colors, _ = bp_case(V, R, 77)
    depth[1] = np.random.default_rng(1).uniform(0.5, 1.8, (R, R)).astype(F)            # (a view with nothing in it has no round trip)
    d, c = on(dev, depth, F), on(dev, cams, F)
    cloud, counts, rank = ops.backproject(d, c, float(FOCAL), Z_MIN, Z_MAX, colors=on(dev, colors, F), want_rank=True)
    counts, rank_h = host(counts), host(rank)
    for v in range(V):
        lo, hi = int(counts[:v].sum()), int(counts[:v + 1].sum())
        dep, idx, _ = ops.splat_points(cloud[None, lo:hi], c[None, v:v + 1], R, float(FOCAL), Z_MIN, Z_MAX, radius=0)
        assert np.array_equal(host(idx)[0, 0], np.where(rank_h[v] >= 0, rank_h[v] - lo, -1))
        ok = rank_h[v] >= 0
        p = host(cloud)[lo:hi, :3]
        scale = np.zeros((R, R))
        scale[ok] = RC.U24 * (np.abs(p).sum(1) + np.abs(cams[v, :3, 3]).sum())
        err = np.abs(host(dep)[0, 0].astype(np.float64) - np.where(ok, depth[v], 0.0))
        assert (err[ok] <= 16 * scale[ok]).all() and (host(dep)[0, 0][~ok] == 0).all()
    got = tuple(host(t) for t in ops.splat_points(cloud[None], c[None], R, float(FOCAL), Z_MIN, Z_MAX, radius=0))
    assert_picture(got, RC.splat32(host(cloud)[None], cams[None], R, FOCAL, Z_MIN, Z_MAX, 0), "the fused cloud into every camera")


def test_render_pcl_of_a_small_generator(dev):
    """SHORTSIREN, hidden 64, R = 16, 12 + 12 samples, 3 views: the cloud is fuse_depth_maps of the generator's own outputs (same seed, same
    draws), n is the number of depth pixels strictly inside (ray_start, ray_end), and the cloud goes into the other shape entries."""
    import global_latent_common as GL
    from cnerf_amd import ops, views, voxels
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix
    gen = GL.fresh_generator(64, seed=3).to(dev)
    gen.set_device(dev)
    z = torch.randn(1, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    origins = torch.tensor([[0.0, 0.3, 1.0], [0.9, 0.2, -0.4], [-0.6, -0.5, 0.7]])
    cams = create_cam2world_matrix(origins, "y").to(dev)
    kw = dict(hierarchical_sample=True, clamp_mode="relu", nerf_noise=0.0, white_back=True)
    R, S = 16, 12
    torch.manual_seed(5)
    cloud = views.render_pcl(gen, z, cams, R, FOV, Z_MIN, Z_MAX, S, **kw)
    torch.manual_seed(5)
    with torch.no_grad():
        img, dep = gen(z.expand(3, -1), cams, img_size=R, fov=FOV, ray_start=Z_MIN, ray_end=Z_MAX, num_steps=S, **kw)
    assert torch.equal(cloud, views.fuse_depth_maps(img, dep, cams, FOV, Z_MIN, Z_MAX))
    n = int(((dep > Z_MIN) & (dep < Z_MAX)).sum())
    assert cloud.shape == (n, 6) and n > 0 and not cloud.requires_grad
    want = RC.backproject32(host(dep), host(cams), FOCAL, Z_MIN, Z_MAX, colors=host(img), color_scale=0.5, color_offset=0.5)[0]
    assert RC.same_bits(host(cloud), want)
    some = views.render_pcl(gen, z, cams, R, FOV, Z_MIN, Z_MAX, S, views_per_batch=2, **kw)      # two batches: other draws, the same kind of cloud
    assert some.dim() == 2 and some.shape[1] == 6 and bool(torch.isfinite(some).all())
    d2, idx = ops.nearest_points(cloud[:, :3].contiguous(), cloud[:, :3].contiguous())
    assert bool(torch.isfinite(d2).all()) and idx.shape == (n,)
    vox = voxels.voxelize_cloud(cloud[None], 16, 2.4)
    assert vox.shape == (1, 4, 16, 16, 16) and 0 < int(vox[0, 0].sum()) <= n
    image, depth, index = views.splat_cloud(cloud[None], cams[None], R, FOV, 0.1, 2.5, radius=0)     # (bounds wide of the depths' own)
    assert image.shape == (1, 3, 3, R, R) and depth.shape == (1, 3, R, R) and int((index >= 0).sum()) >= n


def trainer(dev, **extra):
    from cnerf_amd.training import GanTrainer, default_metadata
    torch.manual_seed(0)
    np.random.seed(0)
    md = default_metadata(img_size=32, num_steps=12, batch_size=2, batch_split=1, hidden_dim=64)
    md["unet"].update(f_maps=8, num_levels=3)
    md["generator"]["z_dim"] = 32
    md["dataset"] = {"voxelize_pcl": True}
    md.update(voxel_resolution=32, **extra)
    return GanTrainer(md, dev)


def test_trainer_depth_term(dev):
    """One generator step at the configuration of test_trainer_voxelises_the_clouds_of_a_step, the target splatted from sample["pcl"]:
    last["depth_loss"] is loss_depth of that splat and the step's own depth output.  With the key off (absent is read as off) the
    step reports the same losses, bit for bit, and no depth term."""
    from cnerf_amd import views
    from cnerf_amd.training import loss_depth
    from cnerf_amd.training.gan_step import synthetic_sample
    sample = synthetic_sample(2, 32, 32, dev, torch.Generator().manual_seed(1), pcl_points=2048)

    def g_step(**extra):
        tr = trainer(dev, **extra)
        seen = []
        tr.generator.register_forward_hook(lambda m, args, out: seen.append(out[1].detach().clone()))
        tr.set_alpha()
        torch.manual_seed(11)
        tr.train_generator(sample)
        torch.cuda.synchronize()
        return tr, seen

    tr, seen = g_step(depth_loss=True, depth_loss_weight=0.5, depth_splat_radius=2)
    md = tr.metadata
    target = views.splat_cloud(sample["pcl"], sample["cam2world"], 32, md["fov"], md["ray_start"], md["ray_end"], radius=2)[1][:, 0]
    assert len(seen) == 1 and seen[0].shape == target.shape == (2, 32, 32)
    fg = float((target != 0).float().mean())
    assert 0.05 < fg <= 1.0
    got = tr.last["depth_loss"]
    assert np.isfinite(got) and got > 0 and got == loss_depth(target, seen[0]).item()
    assert all(np.isfinite(tr.last[k]) for k in ("g_loss", "photo_loss", "g_grad_norm", "e_grad_norm"))
    given = torch.full_like(target, 0.75)                            # a batch that brings its depth images: they are the target, no splat
    assert torch.equal(tr._depth_target({**sample, "depth": given}, sample["cam2world"]), given)
    assert torch.equal(tr._depth_target(sample, sample["cam2world"]), target)
    off, _ = g_step(depth_loss=False)
    assert "depth_loss" not in off.last and not off.depth_loss
    for k in ("g_loss", "photo_loss"):
        assert off.last[k] == tr.last[k], k                          # the forward is the same; the depth term only adds to the loss
