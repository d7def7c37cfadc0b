"""Depth maps -> a TSDF lattice on the GPU: cnerf_tsdf_integrate through ops (and once through ctypes alone, on a second stream) against
its NumPy statement (tests/tsdf_common.py), bit for bit on every output; then the pieces around it -- views.tsdf_volume into
ops.isosurface, extract_shapes.extract_mesh_tsdf on a stand-in generator, shape_metrics.mesh_metrics -- on the analytic ball.
The lattices are a few thousand to 36,000 points, but for one of 64^3 with 12 views of 128^2."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import isosurface_common as IC
import reproject_common as RC
import tsdf_common as TC
from test_gpu_isosurface import assert_mesh_equals
from test_gpu_reproject import bp_case

pytestmark = pytest.mark.gpu

F = np.float32
Z_MIN, Z_MAX = 0.25, 1.95                                    # bp_case's bounds
FOCAL = RC.focal32()
FOV = 49.134342641202636
TRUNC = F(0.15)
INSIDE = RC.look_at([[0.004, 0.02, -0.2]])[0]                # a camera inside every lattice box below: voxels behind it have z <= 0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def on(dev, a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def host(t):
    return None if t is None else t.cpu().numpy()


def box(shape):
    """A box about the origin whose longest edge is 1.2: pitch, and the corner lo."""
    pitch = F(1.2 / (max(shape) - 1))
    return tuple(F(-0.5 * (n - 1)) * pitch for n in shape), pitch


def views_case(V, R, seed):
    """The depth mixture of test_gpu_reproject.bp_case: view 0 holds depths inside, below, above, exactly z_min, exactly z_max, 0, NaN and
    both infinities; view 1 (V = 5) has no surface pixel; the last view only surface pixels.  With V = 5, camera 2 stands inside the box."""
    depth, cams, colors, _ = bp_case(max(V, 3), R, seed)
    depth, cams, colors = depth[:V].copy(), cams[:V].copy(), colors[:V].copy()
    if V == 5:
        cams[2] = INSIDE
    return depth, cams, colors


def gpu_tsdf(dev, shape, lo, pitch, depth, cams, trunc=TRUNC, colors=None, color_layout=0, want_weight=True, **kw):
    from cnerf_amd import ops
    t, w, c = ops.tsdf_integrate(on(dev, depth, F), on(dev, cams, F), float(FOCAL), Z_MIN, Z_MAX, shape, [float(x) for x in lo], float(pitch), float(trunc),
                                 colors=on(dev, colors, F), color_layout={0: "chw", 1: "hwc"}[color_layout], want_weight=want_weight, **kw)
    assert t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and not t.requires_grad
    assert (w is None) == (not want_weight) and (c is None) == (colors is None)
    assert w is None or (w.dtype == torch.int32 and tuple(w.shape) == tuple(shape))
    assert c is None or (c.dtype == torch.float32 and tuple(c.shape) == tuple(shape) + (3,))
    return host(t), host(w), host(c)


FLAGS = list(itertools.product((True, False), (0, 1, 2), (-1.0, 0.25)))          # carve, hidden_min, unseen


@pytest.mark.parametrize("shape,V,R", [((2, 2, 2), 1, 16), ((2, 2, 2), 5, 33), ((5, 7, 67), 5, 16), ((33, 33, 33), 5, 33), ((33, 33, 33), 1, 16),
                                       ((3, 130, 65), 5, 16), ((3, 130, 65), 1, 33)])
def test_tsdf_equals_the_statement(dev, shape, V, R):
    """(2,2,2): eight voxels, one partly filled wave.  (5,7,67): 2,345 voxels, i2 runs of 67 that straddle waves and blocks.  (33,33,33):
    35,937 = 140 blocks of 256 and 97 voxels.  (3,130,65): 25,350, a short slowest axis.  Every combination of carve, hidden_min in
    {0,1,2} and unseen in {-1, 0.25}; the colour mode (none, chw, hwc -- the latter two with scale and offset 0.5) and the weight output
    rotate through them."""
    depth, cams, colors = views_case(V, R, 3 * V + R + shape[2])
    hwc = np.ascontiguousarray(colors.transpose(0, 2, 3, 1))
    lo, pitch = box(shape)
    kinds = set()
    for k, (carve, hidden_min, unseen) in enumerate(FLAGS):
        mode = k % 3
        ckw = {} if mode == 0 else dict(colors=colors if mode == 1 else hwc, color_layout=mode - 1, color_scale=0.5, color_offset=0.5)
        want = TC.tsdf32(shape, lo, pitch, depth, cams, FOCAL, Z_MIN, Z_MAX, TRUNC, carve=carve, hidden_min=hidden_min, unseen=unseen, **ckw)
        got = gpu_tsdf(dev, shape, lo, pitch, depth, cams, carve=carve, hidden_min=hidden_min, unseen=unseen, want_weight=k % 2 == 0, **ckw)
        what = (shape, V, R, carve, hidden_min, unseen, mode)
        assert RC.same_bits(got[0], want[0]), what
        if got[1] is not None:
            assert np.array_equal(got[1], want[1]), what
        if mode:
            assert RC.same_bits(got[2], want[2]), what
            kinds.add("colour" if (want[2] != 0).any() else "")
        w = want[1]
        kinds |= {name for name, hit in (("seen", (w > 0).any()), ("hidden", (w < 0).any()), ("nothing", (w == 0).any()),
                                         ("solid", ((w < 0) & (want[0] == 1)).any()), ("unseen", (want[0] == F(unseen)).any())) if hit}
    if max(shape) > 2:                                                         # the inputs reach every branch
        pos = IC.positions(shape, lo, pitch).reshape(-1, 3)
        zs = [RC.project32(pos, cams[w], FOCAL, R) for w in range(V)]
        with np.errstate(invalid="ignore"):
            assert any(((z > 0) & ~((u > -1) & (u < R) & (v > -1) & (v < R))).any() for z, u, v in zs)             # outside an image
            assert V == 1 or (zs[2][0] <= 0).any()                                                                  # behind the camera inside the box
        assert {"seen", "hidden", "nothing", "solid", "unseen"} <= kinds and (V == 1 or "colour" in kinds), kinds
    if V == 5:
        assert not ((Z_MIN < depth[1]) & (depth[1] < Z_MAX)).any()              # a view with no surface pixel
    for val in (Z_MIN, Z_MAX, 0.0, np.inf, -np.inf):
        assert (depth[0] == F(val)).any()
    assert np.isnan(depth[0]).any()


def test_a_larger_lattice_and_two_runs(dev):
    """(64,64,64) with 12 views of 128^2: 1,024 blocks, every view but the first two of bp_case's mixture; then the same call again."""
    shape, V, R = (64, 64, 64), 12, 128
    depth, cams, colors = views_case(V, R, 11)
    cams[5] = INSIDE
    lo, pitch = box(shape)
    kw = dict(colors=colors, color_layout=0, color_scale=0.5, color_offset=0.5, hidden_min=2)
    want = TC.tsdf32(shape, lo, pitch, depth, cams, FOCAL, Z_MIN, Z_MAX, TRUNC, **kw)
    a = gpu_tsdf(dev, shape, lo, pitch, depth, cams, **kw)
    b = gpu_tsdf(dev, shape, lo, pitch, depth, cams, **kw)
    assert RC.same_bits(a[0], want[0]) and np.array_equal(a[1], want[1]) and RC.same_bits(a[2], want[2])
    assert RC.same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and RC.same_bits(a[2], b[2])
    assert (want[1] > 0).any() and (want[1] < 0).any() and (want[2] != 0).any()


def test_through_ctypes_alone_on_a_second_stream(dev):
    """The C entry with caller-made buffers on a stream of its own.  tsdf is the head of one sentinel-filled buffer: with weight and rgb
    NULL (colours given) nothing behind the lattice's n floats is written; then with every output given."""
    from cnerf_amd import _lib as L
    lib = L.lib()
    shape, V, R = (5, 7, 67), 5, 16
    n = int(np.prod(shape))
    depth, cams, colors = views_case(V, R, 21)
    lo, pitch = box(shape)
    want = TC.tsdf32(shape, lo, pitch, depth, cams, FOCAL, Z_MIN, Z_MAX, TRUNC, colors=colors, color_scale=0.5, color_offset=0.5)
    d, cm, co = on(dev, depth, F), on(dev, cams.reshape(V, 16), F), on(dev, colors, F)
    lo3 = (C.c_float * 3)(*[float(x) for x in lo])
    stream = torch.cuda.Stream(device=dev)
    buf = torch.full((5 * n + 64,), 12345.0, dtype=torch.float32, device=dev)
    wgt = torch.full((n + 64,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)

    def call(weight, rgb):
        L.check(lib.cnerf_tsdf_integrate(*shape, lo3, float(pitch), V, R, L.ptr(d), L.ptr(co), 0, 0.5, 0.5, L.ptr(cm), float(FOCAL), Z_MIN, Z_MAX,
                                         float(TRUNC), 1, 1, -1.0, L.ptr(buf), weight, rgb, C.c_void_p(stream.cuda_stream)), "tsdf_integrate")
        stream.synchronize()

    call(None, None)
    got = host(buf)
    assert RC.same_bits(got[:n], want[0].reshape(-1)) and (got[n:] == 12345.0).all()
    assert (host(wgt) == -77).all()
    rgb = buf[n + 32:]                                                          # 4 n + 32 floats: the colours, and sentinels behind them
    call(L.ptr(wgt), C.c_void_p(rgb.data_ptr()))
    got, gw = host(buf), host(wgt)
    assert RC.same_bits(got[:n], want[0].reshape(-1)) and (got[n:n + 32] == 12345.0).all()
    assert RC.same_bits(got[n + 32:4 * n + 32], want[2].reshape(-1)) and (got[4 * n + 32:] == 12345.0).all()
    assert np.array_equal(gw[:n], want[1].reshape(-1)) and (gw[n:] == -77).all()


def test_ops_refuses(dev):
    from cnerf_amd import _lib, ops
    depth, cams, colors = views_case(5, 16, 1)
    d, c, co = on(dev, depth, F), on(dev, cams, F), on(dev, colors, F)
    ok = dict(shape=(4, 5, 6), lo=(-0.5, -0.5, -0.5), pitch=0.2, trunc=0.3)
    ops.tsdf_integrate(d, c, 2.18, Z_MIN, Z_MAX, **ok)
    for kw in (dict(ok, shape=(4, 5)), dict(ok, shape=(1, 5, 6)), dict(ok, shape=(4, 5, 1025)), dict(ok, pitch=0.0), dict(ok, trunc=0.0),
               dict(ok, lo=(0.0, float("nan"), 0.0)), dict(ok, hidden_min=-1), dict(ok, unseen=float("inf")), dict(ok, colors=co, color_layout="hwc"),
               dict(ok, color_layout="nchw")):
        with pytest.raises(_lib.CnerfError):
            ops.tsdf_integrate(d, c, 2.18, Z_MIN, Z_MAX, **kw)
    for args in ((d, c[:2], 2.18, Z_MIN, Z_MAX), (d, c, 0.0, Z_MIN, Z_MAX), (d, c, 2.18, Z_MAX, Z_MIN), (d[:, :4], c, 2.18, Z_MIN, Z_MAX)):
        with pytest.raises(_lib.CnerfError):
            ops.tsdf_integrate(*args, **ok)


# ---------------------------------------------------------------------------------------------------------------------
# the analytic ball through the pieces around the kernel
# ---------------------------------------------------------------------------------------------------------------------
N, R, V, SIDE, BALL_R = 32, 64, 8, 0.9, 0.35
RAY_START, RAY_END = 0.5, 2.5


def ball_views():
    cams = RC.cameras(V, 5, 1.4, 1.6)
    return cams, TC.sphere_pixels(cams, R, FOCAL, BALL_R), TC.sphere_depth(cams, R, FOCAL, BALL_R)


class BallGenerator:
    """Stands in for a generator: returns the analytic ball's pixels and depth for the cameras it is given."""

    def __init__(self, device):
        self.device = device
        self.calls = []

    def __call__(self, z, cam2worlds, img_size, fov, ray_start, ray_end, num_steps, **kw):
        cams = cam2worlds.cpu().numpy()
        self.calls.append((tuple(z.shape), len(cams), kw))
        return on(self.device, TC.sphere_pixels(cams, img_size, FOCAL, BALL_R)), on(self.device, TC.sphere_depth(cams, img_size, FOCAL, BALL_R))


def test_tsdf_volume_then_isosurface_equals_the_statements(dev):
    from cnerf_amd import ops, views
    cams, pixels, depth = ball_views()
    tsdf, weight, rgb, lo, pitch = views.tsdf_volume(on(dev, pixels), on(dev, depth), on(dev, cams), FOV, RAY_START, RAY_END, resolution=N, cube_length=SIDE,
                                                     want_weight=True)
    assert lo == (-SIDE / 2,) * 3 and pitch == SIDE / (N - 1)
    trunc = F(3.0 * pitch)                                                     # tsdf_volume's default, rounded as the C call rounds it
    want = TC.tsdf32((N, N, N), lo, pitch, depth, cams, FOCAL, RAY_START, RAY_END, trunc, colors=pixels, color_scale=0.5, color_offset=0.5)
    assert RC.same_bits(host(tsdf), want[0]) and np.array_equal(host(weight), want[1]) and RC.same_bits(host(rgb), want[2])
    got = tuple(host(t) for t in ops.isosurface(tsdf, 0.0, lo=lo, pitch=pitch, attrs=rgb))
    assert_mesh_equals(got, IC.isosurface(want[0], 0.0, lo, pitch, want[2]), "tsdf ball")
    v, f, c = got
    assert IC.edge_census(f) == (1, 0) and IC.euler_characteristic(len(v), f) == 2 and IC.signed_volume(v, f) > 0
    assert np.abs(np.linalg.norm(v, axis=1) - BALL_R).max() <= 1.5 * pitch
    # the colour is 0.5 normal + 0.5 of the ball where the views saw it: close to the vertex's own direction
    want_c = 0.5 * v / np.linalg.norm(v, axis=1, keepdims=True) + 0.5
    assert np.abs(c - want_c).mean() < 0.1


def test_extract_mesh_tsdf_and_mesh_metrics(dev):
    from cnerf_amd import extract_shapes, ops, shape_metrics, views
    gen = BallGenerator(dev)
    z = torch.zeros((1, 4), device=dev)
    cams = on(dev, RC.cameras(V, 5, 1.4, 1.6))
    kw = dict(voxel_resolution=N, cube_length=SIDE)
    v, f, c = extract_shapes.extract_mesh_tsdf(gen, z, cams, R, FOV, RAY_START, RAY_END, 12, views_per_batch=3, clamp_mode="relu", **kw)
    assert [(s, k) for s, k, _ in gen.calls] == [((3, 4), 3), ((3, 4), 3), ((2, 4), 2)] and all(k == dict(clamp_mode="relu") for _, _, k in gen.calls)
    # the same composition by hand
    _, pixels, depth = ball_views()
    tsdf, _, rgb, lo, pitch = views.tsdf_volume(on(dev, pixels), on(dev, depth), cams, FOV, RAY_START, RAY_END, resolution=N, cube_length=SIDE)
    hv, hf, hc = ops.isosurface(tsdf, 0.0, lo=lo, pitch=pitch, attrs=rgb)
    assert torch.equal(v, hv) and torch.equal(f, hf) and torch.equal(c, hc) and len(f) > 1000
    v2, f2, c2 = extract_shapes.extract_mesh_tsdf(gen, z, cams, R, FOV, RAY_START, RAY_END, 12, colors=False, **kw)
    assert c2 is None and torch.equal(v2, v) and torch.equal(f2, f)
    # scored like any mesh: a cloud on the sphere, tau of two pitches
    rng = np.random.default_rng(0)
    cloud = rng.normal(size=(20000, 3))
    cloud = (BALL_R * cloud / np.linalg.norm(cloud, axis=1, keepdims=True)).astype(F)
    scores = shape_metrics.mesh_metrics(v, f, on(dev, cloud), n_samples=20000, tau=2 * pitch)
    print(scores)
    assert scores["f_score"] > 0.95 and np.isfinite(scores["chamfer_mesh_to_cloud"]) and np.isfinite(scores["chamfer_cloud_to_mesh"])
    assert scores["vertices"] == len(v) and scores["triangles"] == len(f)
