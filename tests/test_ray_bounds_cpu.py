"""Per-ray sampling bounds (cnerf_occupancy_ray_bounds, cnerf_render_rays_bounded_forward / _bounded_masked_forward), no GPU: the host
code's exports and refusals, the ValueErrors of the Python layer, and the float64 statement of the contract (tests/ray_bounds_common.py)
on hand-computed cases and under one-ulp perturbations of its inputs."""
import ctypes

import numpy as np
import pytest
import torch

import ray_bounds_common as BC
import render_rays_common as RC

ENTRIES = ("cnerf_occupancy_ray_bounds", "cnerf_render_rays_bounded_forward", "cnerf_render_rays_bounded_masked_forward")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def rays_cfg(L, S=12):
    cfg = L.Cfg()
    cfg.B, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = 2, S, 8, 32, 64, 4
    for i in range(4):
        cfg.layer_kind[i] = L.LAYER_FILM
    cfg.voxel_length, cfg.ray_start, cfg.ray_end = 1.2, 0.25, 1.95
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, 8, 32
    cfg.precision = L.PREC_FP32
    cfg.flags = L.F_HIERARCHICAL
    return cfg


def occupancy(L, G=8, side=2.0, bits=0x1000):
    oc = L.Occupancy()
    oc.bits, oc.G, oc.side = bits, G, side
    oc.lo[0] = oc.lo[1] = oc.lo[2] = -1.0
    return oc


def test_exports_and_prototypes(L):
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10
    assert [f for f, _ in L.RayBounds._fields_] == ["near", "far"] and ctypes.sizeof(L.RayBounds) == 16
    assert "typedef struct cnerf_ray_bounds" in header
    # nothing that existed changed size
    assert ctypes.sizeof(L.Rays) == 16 and ctypes.sizeof(L.Occupancy) == 32


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message naming the argument; nothing was launched: there is no GPU here, the device pointers are
    made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    rays = L.Rays()
    rays.origins = rays.dirs = 0x1000
    no_origins = L.Rays()
    no_origins.dirs = 0x1000
    vols = L.Volumes()
    vols.level[0] = 0x1000
    rng = L.Rng()
    rng.u_fine = 0x1000
    both = L.RayBounds()
    both.near = both.far = 0x1000
    only_near, only_far = L.RayBounds(), L.RayBounds()
    only_near.near = only_far.far = 0x1000
    ref = lambda s: ctypes.byref(s) if s is not None else None

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def bounded(cfg, r=rays, P=10, b=both, draws=rng):
        return lib.cnerf_render_rays_bounded_forward(ctypes.byref(cfg), ref(r), P, ref(b), ctypes.byref(vols), fake, fake, fake, ref(draws), fake, fake, None,
                                                     fake, None)

    def bounded_masked(cfg, r=rays, P=10, b=both, draws=rng, oc=None):
        oc = occupancy(L) if oc is None else oc
        return lib.cnerf_render_rays_bounded_masked_forward(ctypes.byref(cfg), ref(r), P, ref(b), ref(oc) if oc != "null" else None, ctypes.byref(vols), fake,
                                                            fake, fake, ref(draws), fake, fake, None, None, fake, None)

    for call in (bounded, bounded_masked):
        # what the unbounded entries refuse -- with bounds, and with a NULL bounds pointer
        for b in (both, None):
            refused(call(rays_cfg(L), r=None, b=b), "rays is NULL")
            refused(call(rays_cfg(L), r=no_origins, b=b), "origins")
            refused(call(rays_cfg(L), P=0, b=b), "rays_per_image")
            refused(call(rays_cfg(L, S=1), b=b), "S=1")
            refused(call(rays_cfg(L, S=129), b=b), "S=129")
            cfg = rays_cfg(L)
            cfg.drop_p = 0.25
            refused(call(cfg, b=b), "dropout")
            refused(call(rays_cfg(L), draws=None, b=b), "u_fine")
        # only one of the two arrays
        refused(call(rays_cfg(L), b=only_near), "bounds.near", "bounds.far")
        refused(call(rays_cfg(L), b=only_far), "bounds.near", "bounds.far")
        assert "bounded" in lib.cnerf_last_error().decode()
    # the grid checks of the masked entry
    refused(bounded_masked(rays_cfg(L), oc="null"), "occupancy is NULL")
    for G in (0, 6, 260):
        refused(bounded_masked(rays_cfg(L), oc=occupancy(L, G=G)), f"G={G}")
    refused(bounded_masked(rays_cfg(L), oc=occupancy(L, side=0.0)), "side")
    refused(bounded_masked(rays_cfg(L), oc=occupancy(L, bits=None)), "bits is NULL")

    def bounds(oc=None, r=rays, B=2, P=10, t_min=0.25, t_max=1.95, pad=0.0, near=fake, far=fake):
        oc = occupancy(L) if oc is None else oc
        return lib.cnerf_occupancy_ray_bounds(ref(oc) if oc != "null" else None, ref(r), B, P, t_min, t_max, pad, near, far, None, None)

    refused(bounds(oc="null"), "occupancy is NULL")
    for G in (0, 3, 6, 10, 260, -4):
        refused(bounds(oc=occupancy(L, G=G)), f"G={G}")
    for side in (0.0, -2.0, float("nan"), float("inf")):
        refused(bounds(oc=occupancy(L, side=side)), "side")
    refused(bounds(oc=occupancy(L, bits=None)), "bits is NULL")
    refused(bounds(r=None), "rays is NULL")
    refused(bounds(r=no_origins), "origins")
    refused(bounds(B=0), "B=0")
    refused(bounds(P=0), "rays_per_image")
    for pad in (-0.125, float("nan"), float("inf")):
        refused(bounds(pad=pad), "pad")
    refused(bounds(t_min=1.0, t_max=1.0), "t_max", "t_min")
    refused(bounds(t_min=1.95, t_max=0.25), "t_max", "t_min")
    refused(bounds(t_max=float("nan")), "t_max")
    refused(bounds(t_min=float("-inf")), "t_min")
    refused(bounds(near=None), "near")
    refused(bounds(far=None), "far")


def test_python_layer_refuses_half_given_and_misshapen_bounds(L):
    """ValueError before any device work (CPU tensors throughout): one of ray_near / ray_far alone, a shape other than (B,P), a grid for
    another batch."""
    from cnerf_amd import ops
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 5, 4, seed=1)
    z = (case.vols[0], case.glob)
    args = (z, case.origins, case.dirs, RC.RAY_START, RC.RAY_END, 4, True)
    kw = dict(clamp_mode="relu", nerf_noise=0.0)
    near, far = torch.full((2, 5), 0.5), torch.full((2, 5), 1.5)
    with torch.no_grad():
        with pytest.raises(ValueError, match="both"):
            case.gen.render_rays(*args, ray_near=near, **kw)
        with pytest.raises(ValueError, match="both"):
            case.gen.render_rays(*args, ray_far=far, **kw)
        for bad in (near[:, :4], near[:1], near.reshape(2, 5, 1), near.reshape(-1)):
            with pytest.raises(ValueError, match="B,P"):
                case.gen.render_rays(*args, ray_near=bad, ray_far=far, **kw)
            with pytest.raises(ValueError, match="B,P"):
                case.gen.render_rays(*args, ray_near=near, ray_far=bad, **kw)
        net = case.gen.siren
        o_args = (net, case.vols[0], None, None, case.origins, case.dirs, RC.RAY_START, RC.RAY_END, 4, True, "relu", 0.0)
        with pytest.raises(ValueError, match="both"):
            ops.render_rays(*o_args, near=near)
        with pytest.raises(ValueError, match="B,P"):
            ops.render_rays(*o_args, near=near, far=far[:, :3])
        grid = ops.OccupancyGrid(torch.zeros((3, 16), dtype=torch.int32), (-1.0,) * 3, 2.0, 8)
        with pytest.raises(ValueError, match="grids"):
            case.gen.ray_bounds(grid, case.origins, case.dirs, RC.RAY_START, RC.RAY_END)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement of the contract
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_on_hand_computed_cases():
    """lo = -1, side = 2, G = 8 (cell edge 0.25).  The numbers are worked out here, by hand, from the cell edges."""
    G, lo, side = 8, [-1.0] * 3, 2.0
    cells = np.zeros((G, G, G), bool)
    one = lambda o, d, t_min=0.25, t_max=4.0, pad=0.0: tuple(float(v[0]) for v in BC.bounds_of(np.array([o], np.float32), np.array([d], np.float32),
                                                                                             cells.reshape(-1), lo, side, G, t_min, t_max, pad))
    # an axis-parallel ray through cell centres: cells 2..4 of the row y, z in [0, 0.25] span x in [-0.5, 0.25], reached at t = 1.5 .. 2.25
    cells[2:5, 4, 4] = True
    assert one([-2, 0.125, 0.125], [1, -0.0, 0.0]) == (1.5, 2.25, 1.0)
    assert one([-2, 0.125, 0.125], [2, 0.0, 0.0]) == (0.75, 1.125, 1.0)                 # depths are in units of |dir|
    assert one([-2, 0.125, 0.125], [1, 0, 0], pad=0.125) == (1.375, 2.375, 1.0)
    assert one([-2, 0.125, 0.125], [1, 0, 0], t_min=1.75, t_max=2.0, pad=0.5) == (1.75, 2.0, 1.0)       # clamped to [t_min, t_max]
    assert one([-2, 0.375, 0.125], [1, 0, 0]) == (0.25, 4.0, 0.0)                       # the row next to it: T is empty
    # a span that is not convex: the hull runs from the first set cell to the last
    cells[7, 4, 4] = True
    assert one([-2, 0.125, 0.125], [1, 0, 0]) == (1.5, 3.0, 1.0)
    cells[7, 4, 4] = False
    # a diagonal through the cube: it enters at t = 0.5 and crosses cell (k,k,k) over [0.5 + 0.25 k, 0.75 + 0.25 k]
    cells[:] = False
    cells[2, 2, 2] = cells[5, 5, 5] = True
    assert one([-1.5, -1.5, -1.5], [1, 1, 1]) == (1.0, 2.0, 1.0)
    cells[6, 6, 7] = True                                       # closed cells: touched in the one point (0.75, 0.75, 0.75), t = 2.25
    assert one([-1.5, -1.5, -1.5], [1, 1, 1]) == (1.0, 2.25, 1.0)
    cells[:] = False
    cells[6, 6, 7] = True                                       # ... and touched there only: far <= near, a miss
    assert one([-1.5, -1.5, -1.5], [1, 1, 1]) == (0.25, 4.0, 0.0)
    assert one([-1.5, -1.5, -1.5], [1, 1, 1], pad=0.25) == (2.0, 2.5, 1.0)
    # a miss: every cell set, the ray passes beside the cube / points away from it / is parallel to a face outside the slab
    cells[:] = True
    assert one([-2, 3, 0], [1, 0, 0]) == (0.25, 4.0, 0.0)
    assert one([-2, 0, 0], [-1, 0.1, 0]) == (0.25, 4.0, 0.0)
    assert one([-2, 0, 0], [1, 0, 0]) == (1.0, 3.0, 1.0)
    assert one([0, 0, 0], [0, 0, 0]) == (0.25, 4.0, 1.0)        # a ray that does not move sits in its cell for every t
    # a ray starting inside a set cell: near is t_min; it leaves cell (4,4,4) through y = 0.25 at t = 0.125
    cells[:] = False
    cells[4, 4, 4] = True
    assert one([0.125, 0.125, 0.125], [-0.0, 1, 0], t_min=0.0625) == (0.0625, 0.125, 1.0)
    assert one([0.125, 0.125, 0.125], [-0.0, 1, 0], t_min=0.125) == (0.125, 4.0, 0.0)   # only the exit point is left: a miss
    assert one([0.125, 0.125, 0.125], [0, 1, 0], t_min=0.1875) == (0.1875, 4.0, 0.0)    # t_min beyond the exit
    assert one([0.125, np.nan, 0.125], [0, 1, 0], t_min=0.0625) == (0.0625, 4.0, 0.0)   # a NaN anywhere: a miss
    assert one([0.125, 0.125, 0.125], [0, 1, np.nan], t_min=0.0625) == (0.0625, 4.0, 0.0)
    # the shared exact cases carry the same kind of numbers: the reference reproduces them
    o, d, cl, want = BC.exact_cases()
    for pad, (w_near, w_far, w_hit) in want.items():
        for b in range(2):
            near, far, hit = BC.bounds_of(o, d, cl[b], lo, side, G, BC.EXACT_T_MIN, BC.EXACT_T_MAX, pad)
            assert np.array_equal(near, w_near[b]) and np.array_equal(far, w_far[b]) and np.array_equal(hit, w_hit[b].astype(bool)), (pad, b)
    assert want[0.0][2].sum() >= 8 and (want[0.0][2] == 0).sum() >= 6


def one_ulp(a, rng):
    """Every element moved to a float32 neighbour, up or down at random (a NaN stays a NaN, a zero becomes the smallest denormal)."""
    a = np.asarray(a, np.float32)
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, np.float32(-np.inf), np.float32(np.inf))).astype(np.float32)


@pytest.mark.parametrize("side", list(BC.CUBES))
@pytest.mark.parametrize("G", [4, 8, 12])
def test_reference_on_perturbed_inputs_stays_inside_the_sandwich(G, side):
    """The margin delta = 32 * 2^-23 * M of tests/test_gpu_ray_bounds.py's sandwich leaves room for float32 at all: the float64 reference on
    origins and directions moved by one float32 ulp per component -- no more than what reading the inputs in float32 costs -- answers inside
    the sandwich built from the unperturbed inputs, on every ray, pattern and cube of the GPU test."""
    lo = BC.CUBES[side]
    origins, dirs = BC.sandwich_rays(lo, side, 100 * G + int(side * 10))
    rng = np.random.default_rng(G)
    seen_hit = seen_miss = 0
    for kind in BC.PATTERNS:
        for b in range(2):
            cells = BC.pattern_cells(kind, G, seed=G + b)
            delta = BC.delta_of(origins[b], lo, side)
            assert 0 < delta < 1e-5
            inner, outer = BC.sandwich(origins[b], dirs[b], cells, lo, side, G, BC.T_MIN, BC.T_MAX, delta)
            assert not (inner[0] & ~outer[0]).any()
            near, far, hit = BC.bounds_of(one_ulp(origins[b], rng), one_ulp(dirs[b], rng), cells, lo, side, G, BC.T_MIN, BC.T_MAX)
            bad = BC.sandwich_violations(near, far, hit, inner, outer, BC.T_MIN, BC.T_MAX)
            assert not bad, (kind, b, bad[:5])
            seen_hit, seen_miss = seen_hit + int(hit.sum()), seen_miss + int((~hit).sum())
    assert seen_hit > 200 and seen_miss > 200


def test_per_ray_depths_reduce_to_the_scalar_ones():
    """linspace32_rays / bounded_depths with every ray's interval [ray_start, ray_end] are RC.linspace32 / RC.numpy_geometry's depths bit for
    bit; per_ray_depths hands them to the ray oracle and puts the scalar rule back."""
    B, P = 2, 7
    u = np.random.default_rng(0).random((B, P, 12)).astype(np.float32)
    near, far = np.full((B, P), RC.RAY_START, np.float32), np.full((B, P), RC.RAY_END, np.float32)
    o, d = RC.random_rays(B, P, 3)
    for S in (2, 3, 12):
        assert np.array_equal(BC.linspace32_rays(near, far, S)[1, 3], RC.linspace32(RC.RAY_START, RC.RAY_END, S))
        z = BC.bounded_depths(u[..., :S], S, near, far)
        assert np.array_equal(z, RC.numpy_geometry(o.numpy(), d.numpy(), u[..., :S], S, RC.RAY_START, RC.RAY_END)[0])
        assert np.array_equal(z, RC.ray_depths(torch.from_numpy(u[..., :S]), S, RC.RAY_START, RC.RAY_END).numpy())
    n2, f2 = BC.random_bounds(B, P, 5)
    assert (n2 >= np.float32(RC.RAY_START)).all() and (f2 <= np.float32(RC.RAY_END)).all() and ((f2 - n2) < 0.05).any()
    keep = RC.ray_depths
    with BC.per_ray_depths(n2, f2):
        z = RC.ray_depths(torch.from_numpy(u), 12, RC.RAY_START, RC.RAY_END).numpy()
    assert RC.ray_depths is keep and np.array_equal(z, BC.bounded_depths(u, 12, n2, f2))
    zl = BC.linspace32_rays(n2, f2, 12)
    assert np.array_equal(zl[..., 0], n2) and np.array_equal(zl[..., -1], f2) and (np.diff(zl, axis=-1) > 0).all()
