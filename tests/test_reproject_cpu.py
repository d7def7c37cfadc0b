"""Depth maps <-> clouds, no GPU: the host code's exports, workspace sizes and refusals; the NumPy statements of the two contracts
(tests/reproject_common.py) against float64 statements of what the reference computes; the round trip of the two statements; the .obj
writer and the depth loss."""
import ctypes

import numpy as np
import pytest

import reproject_common as RC

ENTRIES = ("cnerf_backproject_bytes", "cnerf_backproject", "cnerf_splat_points_bytes", "cnerf_splat_points")
F = np.float32
U = RC.U24
Z_MIN, Z_MAX = 0.25, 1.95


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def test_exports_and_prototypes(L):
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10 and L.ABI_VERSION == 10 and "#define CNERF_ABI_VERSION 10" in header
    import cnerf_amd
    assert callable(cnerf_amd.ops.backproject) and callable(cnerf_amd.ops.splat_points)
    V = cnerf_amd.views
    assert V.fuse_depth_maps and V.render_pcl and V.splat_cloud and V.write_obj_cloud
    from cnerf_amd.training import loss_depth
    assert callable(loss_depth)


def test_workspace_bytes(L):
    lib = L.lib()
    nb = ctypes.c_size_t(7)
    for B, V, R in ((1, 1, 2), (2, 3, 7), (2, 3, 32), (8, 24, 128), (1, 1, 2048)):
        assert lib.cnerf_splat_points_bytes(B, V, R, ctypes.byref(nb)) == 0, lib.cnerf_last_error()
        need = 8 * B * V * R * R                                         # one 64-bit key per pixel
        assert need <= nb.value < need + 256 and nb.value % 256 == 0
    for V, R in ((1, 2), (3, 5), (3, 33), (6, 128), (24, 128), (1, 2048)):
        assert lib.cnerf_backproject_bytes(V, R, ctypes.byref(nb)) == 0, lib.cnerf_last_error()
        need = 4 * (V * -(-R * R // 256) + 1)                            # the scan's counts: one per 256 pixels of a view, and the total
        assert need <= nb.value < need + 256 and nb.value % 256 == 0
    assert lib.cnerf_backproject_bytes(1, 2, None) == 0 and lib.cnerf_splat_points_bytes(1, 1, 2, None) == 0


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t()
    nan, inf = float("nan"), float("inf")

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def bp(V=3, R=16, depth=fake, colors=None, layout=0, mask=None, mask_min=0.0, cams=fake, focal=2.1877, z_min=0.25, z_max=1.95, scale=1.0, offset=0.0,
           points=fake, ws=fake):
        return lib.cnerf_backproject(V, R, depth, colors, layout, mask, mask_min, cams, focal, z_min, z_max, scale, offset, points, None, None, None, ws, None)

    pinhole = ((dict(focal=0.0), "focal"), (dict(focal=-1.0), "focal"), (dict(focal=inf), "focal"), (dict(focal=nan), "focal"),
               (dict(z_min=-0.1), "z_min"), (dict(z_min=nan), "z_min"), (dict(z_min=inf), "z_min"),
               (dict(z_max=0.25), "z_max"), (dict(z_max=0.1), "z_max"), (dict(z_max=inf), "z_max"), (dict(z_max=nan), "z_max"))
    for kw, word in ((dict(V=0), "V=0"), (dict(V=-2), "V=-2"), (dict(R=1), "R=1"), (dict(R=2049), "R=2049"), (dict(R=0), "R=0"),
                     (dict(V=512, R=2048), "2^31"), (dict(V=2 ** 29, R=2), "2^31"), *pinhole,
                     (dict(mask_min=nan), "mask_min"), (dict(scale=nan), "color_scale"), (dict(offset=nan), "color_offset"),
                     (dict(layout=2), "color_layout=2"), (dict(layout=-1), "color_layout=-1"),
                     (dict(depth=None), "NULL"), (dict(cams=None), "NULL"), (dict(points=None), "NULL"), (dict(ws=None), "NULL")):
        refused(bp(**kw), word)
    for V, R, word in ((0, 8, "V=0"), (1, 1, "R=1"), (1, 2049, "R=2049"), (512, 2048, "2^31")):
        refused(lib.cnerf_backproject_bytes(V, R, ctypes.byref(nb)), word)

    def f3(v):
        return None if v is None else (ctypes.c_float * 3)(*v)

    def sp(B=2, n=100, stride=6, points=fake, n_points=None, V=3, cams=fake, R=16, focal=2.1877, z_min=0.25, z_max=1.95, radius=1, bg=(1.0, 1.0, 1.0),
           depth=fake, index=fake, pixels=fake, ws=fake):
        return lib.cnerf_splat_points(B, n, stride, points, n_points, V, cams, R, focal, z_min, z_max, radius, f3(bg), depth, index, pixels, ws, None)

    for kw, word in ((dict(B=0), "B=0"), (dict(V=0), "V=0"), (dict(n=0), "n=0"), (dict(n=-1), "n=-1"), (dict(n=2 ** 28), "2^28"),
                     (dict(R=1), "R=1"), (dict(R=2049), "R=2049"), (dict(B=1, V=512, R=2048), "2^31"), (dict(B=64, V=8, R=2048), "2^31"),
                     (dict(stride=2), "stride=2"), (dict(stride=0), "stride=0"), (dict(stride=5), "stride=5"), (dict(stride=3), "stride=3"),
                     (dict(radius=-1), "radius=-1"), (dict(radius=9), "radius=9"), *pinhole,
                     (dict(points=None), "NULL"), (dict(cams=None), "NULL"), (dict(ws=None), "NULL"), (dict(bg=None), "background")):
        refused(sp(**kw), word)
    for B, V, R, word in ((0, 1, 8, "B=0"), (1, 0, 8, "V=0"), (1, 1, 1, "R=1"), (2, 256, 2048, "2^31")):
        refused(lib.cnerf_splat_points_bytes(B, V, R, ctypes.byref(nb)), word)


# ---------------------------------------------------------------------------------------------------------------------
# the statements against the reference's arithmetic in float64
# ---------------------------------------------------------------------------------------------------------------------
def depth_maps(V, R, seed, holes=True):
    """Depths mostly inside (Z_MIN, Z_MAX), with pixels below, above, exactly on both bounds, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 1.8, (V, R, R)).astype(F)
    if holes:
        kind = rng.integers(0, 24, (V, R, R))
        for k, val in enumerate((0.1, 2.5, Z_MIN, Z_MAX, np.nan, np.inf, -np.inf, 0.0)):
            d[kind == k] = val
    return d


def test_backproject32_equals_the_reference_lift_in_float64():
    """Roundings on the path of world_i = ((M_i0 xc + M_i1 yc) + M_i2 z) + M_i3: xn one (the quotient; its operands are exact integers),
    xn / focal one, * z one -- three in xc, and as many in yc; each product one; then three sums, each of which perturbs what it
    has summed so far.  So the addend M_i0 xc carries 3 + 1 + 3 = 7 roundings, M_i1 yc 7, M_i2 z 1 + 2 = 3, M_i3 1, and
    |world_i - world64_i| <= 2^-24 (7 |M_i0 xc| + 7 |M_i1 yc| + 3 |M_i2 z| + |M_i3|) to first order; the second-order terms (21 u^2) and
    the float64 side's own 2^-53 are covered by the factor 1.001.  That is below the issue's 8 2^-24 times the plain sum, which is
    asserted as well."""
    worst = 0.0
    for V, R, seed in ((4, 33, 1), (3, 128, 2), (5, 16, 3)):
        depth, cams, focal = depth_maps(V, R, seed), RC.cameras(V, seed), RC.focal32()
        pts, counts, pixel, rank = RC.backproject32(depth, cams, focal, Z_MIN, Z_MAX)
        world, terms = RC.backproject64(depth, cams, focal, Z_MIN, Z_MAX)
        assert len(pts) == counts.sum() == len(world) and 0.5 * depth.size < len(pts) < depth.size
        err = np.abs(pts.astype(np.float64) - world)
        own = 1.001 * U * (terms * np.asarray([7.0, 7.0, 3.0, 1.0])).sum(-1)
        issue = 8 * U * terms.sum(-1)
        worst = max(worst, float((err / own).max()))
        print(f"V={V} R={R}: n={len(pts)}, max err / own bound {float((err / own).max()):.3f}, / the issue's {float((err / issue).max()):.3f}")
        assert (err <= own).all() and (err <= issue).all()
        assert (rank.reshape(-1)[pixel] == np.arange(len(pts))).all() and (rank >= 0).sum() == len(pts)
    assert worst > 0.01


def splat_scene(R, seed=11, B=2, n=5000, V=2):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-0.5, 0.5, (B, n, 3)).astype(F)
    import torch
    import __graft_entry__  # noqa: F401  (puts the repository root on the path)
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix
    d = rng.normal(size=(B * V, 3))
    d[:, 1] *= 0.5                                                   # away from the poles of the look-at
    origins = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.9, 1.3, (B * V, 1))
    cams = create_cam2world_matrix(torch.from_numpy(origins.astype(F)), "y").numpy().reshape(B, V, 4, 4)
    return pts, cams


def z_bound(p, M):
    """Rounding bound of the float32 z = (q0 M02 + q1 M12) + q2 M22, q = p - t: the first two addends carry the subtraction, the product
    and two sums (4 roundings), the third the subtraction, the product and one sum (3): 2^-24 (4 |q0 M02| + 4 |q1 M12| + 3 |q2 M22|),
    to first order (factor 1.001 for the rest); q itself is also perturbed relative to |p| + |t| >= |q|, which the bound uses."""
    p, M = np.asarray(p, np.float64), np.asarray(M, np.float64)
    mag = (np.abs(p[:, :3]) + np.abs(M[:3, 3])) * np.abs(M[:3, 2])
    return 1.001 * U * (mag * np.asarray([4.0, 4.0, 3.0])).sum(-1)


@pytest.mark.parametrize("R", [16, 128])
@pytest.mark.parametrize("radius", [0, 1])
def test_splat32_equals_the_float64_projection(R, radius):
    """2 x 5,000 uniform points in [-0.5, 0.5]^3, two look-at cameras per image at radius 0.9 - 1.3.  Points whose float64 u or v lies
    within 2^-20 R of a half-integer in one of their image's views may round to either pixel in float32 and are removed from the input
    of both sides (at most 1 %); so are points whose float64 z lies within its rounding bound of z_min or z_max.  Then index agrees
    exactly, except at pixels where the two sides' winners have float64 depths that differ by no more than the sum of the two
    points' rounding bounds of z (either order is then possible in float32): at most 0.1 % of the covered pixels.  depth agrees
    within the winner's bound (plus the winners' float64 difference at an excepted pixel)."""
    pts, cams = splat_scene(R)
    focal = RC.focal32()
    B, n, _ = pts.shape
    kept, removed = [], 0
    for b in range(B):
        near = np.zeros(n, bool)
        for w in range(cams.shape[1]):
            z, u, v = RC.project64(pts[b], cams[b, w], focal, R)
            for t in (u, v):
                near |= np.abs((t - 0.5) - np.rint(t - 0.5)) < 2.0 ** -20 * R
            zb = z_bound(pts[b], cams[b, w])
            near |= (np.abs(z - Z_MIN) <= zb) | (np.abs(z - Z_MAX) <= zb)
        removed += near.sum()
        kept.append(pts[b][~near])
    share = removed / (B * n)
    print(f"R={R} radius={radius}: removed {removed} of {B * n} points ({share:.4%})")
    assert share <= 0.01
    m = min(len(k) for k in kept)
    pts = np.stack([k[:m] for k in kept])
    d32, i32, px = RC.splat32(pts, cams, R, focal, Z_MIN, Z_MAX, radius)
    d64, i64, proj = RC.splat64(pts, cams, R, focal, Z_MIN, Z_MAX, radius)
    assert px is None
    covered = excepted = 0
    for b in range(B):
        for w in range(cams.shape[1]):
            z, u, v = proj[b, w]
            inside = (Z_MIN < z) & (z < Z_MAX) & (np.rint(u) >= 0) & (np.rint(u) < R) & (np.rint(v) >= 0) & (np.rint(v) < R)
            assert 0.05 < inside.mean() < 0.95, inside.mean()
            zb = z_bound(pts[b], cams[b, w])
            a, c = i32[b, w].reshape(-1), i64[b, w].reshape(-1)
            assert np.array_equal(a >= 0, c >= 0)
            hit = c >= 0
            differ = hit & (a != c)
            gap = np.abs(z[a[differ]] - z[c[differ]])
            assert (gap <= zb[a[differ]] + zb[c[differ]]).all()
            covered += hit.sum()
            excepted += differ.sum()
            tol = np.where(hit, zb[np.maximum(a, 0)], 0.0)
            tol[differ] += gap
            assert (np.abs(d32[b, w].reshape(-1) - d64[b, w].reshape(-1)) <= tol).all()
            assert (d32[b, w].reshape(-1)[~hit] == 0).all()
    print(f"covered pixels {covered}, excepted {excepted}")
    assert covered > 0 and excepted <= 1e-3 * covered


@pytest.mark.parametrize("R", [8, 16, 33, 64, 128])
def test_round_trip_of_the_two_statements(R):
    """backproject32, then splat32 at radius 0 into the same camera: every valid pixel's point lands on its own pixel and nothing lands
    elsewhere, index == rank on every pixel.  depth within 16 2^-24 (|p|_1 + |t|_1), p the lifted point, t the camera's position.  The
    16 is a count of roundings: 7 on the longest path of the lift (test_backproject32...), then the subtraction of t, the product with
    the rotation's entry and two sums -- 11 -- relative to addends each at most |p|_1 + |t|_1 in sum because a rotation's entries are at
    most 1; the remaining 5 cover that the lift's addends can exceed the coordinates they cancel to.  Measured here: the largest error
    is printed in those units (1.4 to 2.7)."""
    V = 3
    depth, cams, focal = depth_maps(V, R, 40 + R), RC.cameras(V, 50 + R), RC.focal32()
    pts, counts, pixel, rank = RC.backproject32(depth, cams, focal, Z_MIN, Z_MAX)
    worst = 0.0
    for v in range(V):
        lo, hi = counts[:v].sum(), counts[:v + 1].sum()
        d, idx, _ = RC.splat32(pts[None, lo:hi], cams[None, v:v + 1], R, focal, Z_MIN, Z_MAX, 0)
        want = np.where(rank[v] >= 0, rank[v] - lo, -1)
        assert np.array_equal(idx[0, 0], want)
        _, u, w = RC.project32(pts[lo:hi, :3], cams[v], focal, R)
        row, col = np.divmod(pixel[lo:hi] - v * R * R, R)
        assert max(np.abs(u - col).max(), np.abs(w - row).max()) < 1e-3
        ok = rank[v] >= 0
        scale = U * (np.abs(pts[lo:hi, :3]).sum(1) + np.abs(cams[v, :3, 3]).sum())
        err = np.abs(d[0, 0][ok].astype(np.float64) - depth[v][ok]) / scale
        worst = max(worst, float(err.max()))
        assert (err <= 16).all() and (d[0, 0][~ok] == 0).all()
    print(f"R={R}: largest depth error {worst:.2f} x 2^-24 (|p|_1 + |t|_1)")


def test_write_obj_cloud(tmp_path):
    import cnerf_amd
    rng = np.random.default_rng(3)
    cloud = np.concatenate([rng.normal(size=(200, 3)), rng.uniform(-0.2, 1.2, (200, 3))], 1).astype(F)
    cloud[:6, 3:] = np.asarray([[0.0, 1.0, 0.5], [-1.0, 2.0, 1e-9], [1 / 255, 254.5 / 255, 0.999], [0.49999 / 255, 0.5 / 255, 1.5 / 255],
                                [-1e-3, 1.0 + 1e-3, 0.25], [253.5 / 255, 254.49 / 255, 255.5 / 255]], F)
    path = tmp_path / "cloud.obj"
    cnerf_amd.views.write_obj_cloud(str(path), cloud)
    lines = path.read_text().splitlines()
    assert len(lines) == 200 and all(ln.startswith("v ") and len(ln.split()) == 7 for ln in lines)
    got = np.asarray([ln.split()[1:] for ln in lines])
    assert np.array_equal(got[:, :3].astype(np.float64).astype(F), cloud[:, :3])         # str(float32) round-trips
    assert all(a == str(b) for a, b in zip(got[:, 0], cloud[:, 0]))
    # inference.py:562-563,575: pts_color.mul(255).add_(0.5).clamp(0, 255), then astype("uint8") -- float32 throughout
    want = np.clip(cloud[:, 3:] * F(255) + F(0.5), 0, 255).astype(np.uint8)
    assert np.array_equal(got[:, 3:].astype(np.int64), want.astype(np.int64))
    assert want[1].tolist() == [0, 255, 0] and want[0].tolist() == [0, 255, 128] and (want[4, :2] == [0, 255]).all()
    import torch
    cnerf_amd.views.write_obj_cloud(str(path), torch.from_numpy(cloud))                   # a tensor as well
    assert path.read_text().splitlines() == lines
    with pytest.raises(ValueError):
        cnerf_amd.views.write_obj_cloud(str(path), cloud[:, :5])


def test_loss_depth():
    import torch
    from cnerf_amd.training import loss_depth
    gt = torch.tensor([[[0.0, 1.0], [2.0, 0.0]], [[0.0, 0.0], [0.5, 0.0]]])
    pred = torch.tensor([[[9.0, 1.5], [1.0, 9.0]], [[9.0, 9.0], [0.5, 9.0]]], requires_grad=True)
    loss = loss_depth(gt, pred)
    assert loss.item() == pytest.approx((0.25 + 1.0 + 0.0) / 3)
    loss.backward()
    want = torch.zeros_like(gt)
    want[0, 0, 1], want[0, 1, 0] = 2 * 0.5 / 3, 2 * -1.0 / 3
    assert torch.allclose(pred.grad, want)
    # utils.py:96-99 on the same pair
    idx = torch.where(gt != 0)
    assert loss.item() == ((gt[idx] - pred.detach()[idx]) ** 2).mean().item()
    pred.grad = None
    none = loss_depth(torch.zeros_like(gt), pred)                    # all background: 0, and a zero gradient, not a NaN
    assert none.item() == 0.0
    none.backward()
    assert pred.grad is not None and (pred.grad == 0).all()
