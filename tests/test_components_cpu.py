"""Connected components of a lattice (cnerf_components_*), no GPU: the NumPy statement (tests/components_common.py) against
scipy.ndimage.label and against geometry -- the sub-mesh property that makes the 14 Kuhn neighbours the right ones, cavities of a hollow
ball -- and the host code's exports and refusals, in their stated order."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import components_common as CC
import isosurface_common as IC

ENTRIES = ("cnerf_components_bytes", "cnerf_components_label", "cnerf_components_filter")
F = np.float32


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def euler(mesh):
    return IC.euler_characteristic(len(mesh[0]), mesh[1])


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_scipy_as_partitions():
    ndimage = pytest.importorskip("scipy.ndimage")
    cross = ndimage.generate_binary_structure(3, 1)
    kuhn = np.zeros((3, 3, 3), int)
    kuhn[1, 1, 1] = 1
    for d in CC.kinds(14):
        kuhn[1 + d[0], 1 + d[1], 1 + d[2]] = kuhn[1 - d[0], 1 - d[1], 1 - d[2]] = 1
    assert kuhn.sum() == 15 and cross.sum() == 7 and not kuhn[2, 0, 1] and not kuhn[0, 2, 1]      # (1,-1,0) is no kind
    rng = np.random.default_rng(0)
    differ = 0
    for _ in range(30):
        v = rng.standard_normal((7, 6, 5)).astype(F)
        for invert in (False, True):
            sel = CC.selected(v, 0.0, invert)
            l6, l14 = CC.label(v, 0.0, invert, 6)[0], CC.label(v, 0.0, invert, 14)[0]
            assert CC.same_partition(l6, ndimage.label(sel, structure=cross)[0])
            assert CC.same_partition(l14, ndimage.label(sel, structure=kuhn)[0])
            differ += not CC.same_partition(l6, np.where(l14 >= 0, l14 + 1, 0))
    assert differ > 30                                              # the two neighbourhoods are told apart by these lattices


def test_oracle_labels_are_minimum_indices_and_sizes_add_up():
    v = np.random.default_rng(1).standard_normal((9, 8, 7)).astype(F)
    for conn in (6, 14):
        labels, sizes, stats = CC.label(v, 0.2, connectivity=conn)
        lab = labels.ravel()
        on = lab >= 0
        assert np.array_equal(on, (v > 0.2).ravel()) and (lab[on] <= np.nonzero(on)[0]).all() and (lab[lab[on]] == lab[on]).all()
        roots = np.unique(lab[on])
        assert stats[0] == len(roots) and sizes.sum() == on.sum() and np.array_equal(np.nonzero(sizes.ravel())[0], roots)
        assert stats[2] == sizes.max() and stats[1] == np.nonzero(sizes.ravel() == sizes.max())[0][0] and stats[3] == 0
    empty = CC.label(v, 100.0)
    assert (empty[0] == -1).all() and not empty[1].any() and empty[2].tolist() == [0, -1, 0, 0]


def test_checkerboard_is_60_singletons_under_6_and_one_component_under_14():
    v = (np.indices((4, 5, 6)).sum(0) % 2 == 0).astype(F)
    l6, s6, st6 = CC.label(v, 0.5, connectivity=6)
    l14, s14, st14 = CC.label(v, 0.5, connectivity=14)
    assert st6.tolist() == [60, 0, 1, 0] and st14.tolist() == [1, 0, 60, 0]
    assert np.array_equal(l6.ravel()[l6.ravel() >= 0], np.nonzero(v.ravel())[0]) and set(l14.ravel().tolist()) == {-1, 0}


def test_winding_path_is_one_chain():
    w = CC.winding_path()
    assert w.shape == (31, 31, 16) and w.sum() == 16 * 16 * 16 + 255
    for conn in (6, 14):
        assert CC.label(w, 0.5, connectivity=conn)[2].tolist() == [1, 0, 4351, 0]
        assert CC.label(w[::-1, ::-1, ::-1], 0.5, connectivity=conn)[2].tolist() == [1, 0, 4351, 0]
    cut = w.copy()
    cut[14, 30, 7] = 0                                              # the middle of a row: the path falls in two
    assert CC.label(cut, 0.5)[2][0] == 2


# ---------------------------------------------------------------------------------------------------------------------
# why 14: the components are the pieces that the mesh separates
# ---------------------------------------------------------------------------------------------------------------------
def test_filtering_a_ball_and_a_small_ball_leaves_a_submesh():
    N = 24
    pitch = 1.0 / (N - 1)
    v = np.maximum(IC.ball_field((N, N, N), [(0.45, 0.5, 0.5)], 0.3, pitch=pitch), IC.ball_field((N, N, N), [(0.85, 0.8, 0.2)], 0.08, pitch=pitch))
    labels, sizes, stats = CC.label(v, 0.0)
    assert stats[0] == 2 and stats[2] > 10 * (sizes.sum() - stats[2]) > 0
    full = IC.isosurface(v, 0.0, (0, 0, 0), pitch)
    kept = IC.isosurface(CC.keep(v, 0.0), 0.0, (0, 0, 0), pitch)
    assert euler(full) == 4 and euler(kept) == 2 and IC.edge_census(kept[1]) == (1, 0)
    assert 0 < len(kept[1]) < len(full[1]) and CC.is_submesh(kept, full)
    # min_size instead of largest: the same mesh; a finite fill below the level: the same faces
    assert CC.is_submesh(IC.isosurface(CC.keep(v, 0.0, largest=False, min_size=int(stats[2])), 0.0, (0, 0, 0), pitch), kept)
    assert np.array_equal(IC.isosurface(CC.keep(v, 0.0, fill=-1.0), 0.0, (0, 0, 0), pitch)[1], kept[1])


def test_on_noise_the_14_filtered_mesh_is_a_submesh_and_the_6_filtered_one_is_not():
    """12^3 white noise at level 0.3.  Under 14 every component is a piece that the mesh separates; under 6 a solid that hangs together
    by a diagonal is torn apart, the fill lands next to kept points, and new vertices appear."""
    v = np.random.default_rng(5).standard_normal((12, 12, 12)).astype(F)
    full = IC.isosurface(v, 0.3)
    k14, k6 = IC.isosurface(CC.keep(v, 0.3, connectivity=14), 0.3), IC.isosurface(CC.keep(v, 0.3, connectivity=6), 0.3)
    assert CC.label(v, 0.3, connectivity=14)[2][0] > 1 and 0 < len(k14[1]) < len(full[1])
    assert CC.is_submesh(k14, full)
    assert not CC.is_submesh(k6, full)
    # the complement, with the same neighbourhood (at level -0.6, where the outside is what falls apart)
    full = IC.isosurface(v, -0.6)
    o14, o6 = (IC.isosurface(CC.keep(v, -0.6, invert=True, connectivity=c), -0.6) for c in (14, 6))
    assert CC.label(v, -0.6, invert=True)[2][0] > 1 and 0 < len(o14[1]) < len(full[1])
    assert CC.is_submesh(o14, full) and not CC.is_submesh(o6, full)


def test_hollow_ball_cavity_is_filled():
    v, pitch = CC.hollow_ball(24, 0.2, 0.4)
    assert pitch == 1.0 / 23
    full = IC.isosurface(v, 0.0, (0, 0, 0), pitch)
    labels, sizes, stats = CC.label(v, 0.0, invert=True)
    assert euler(full) == 4 and stats[0] == 2 and stats[1] == 0 and stats[3] == 0
    filled = IC.isosurface(CC.keep(v, 0.0, invert=True, fill=1.0), 0.0, (0, 0, 0), pitch)
    ball = 4 / 3 * math.pi * 0.4 ** 3
    V0, V1 = IC.signed_volume(*full[:2]), IC.signed_volume(*filled[:2])
    print("hollow ball: volume", V0, "->", V1, "ball", ball)
    assert euler(filled) == 2 and CC.is_submesh(filled, full) and V0 < V1 and abs(V1 - ball) <= 0.02 * ball


# ---------------------------------------------------------------------------------------------------------------------
# the host code
# ---------------------------------------------------------------------------------------------------------------------
def test_exports_and_prototypes(L):
    header = open(L.HERE + "/../include/cnerf.h").read()
    for name in ENTRIES:
        assert name in L.PROTOTYPES and name + "(" in header
        assert getattr(L.lib(), name).argtypes == L.PROTOTYPES[name][1]
    assert L.lib().cnerf_abi_version() == 10 and "#define CNERF_ABI_VERSION 10" in header
    nb = ctypes.c_size_t()
    assert L.lib().cnerf_components_bytes(256, 256, 256, ctypes.byref(nb)) == 0 and nb.value >= 8


def test_python_layers_have_the_keywords_with_todays_defaults():
    import cnerf_amd
    from cnerf_amd import extract_shapes, ops
    P = lambda f: {k: p.default for k, p in inspect.signature(f).parameters.items()}
    assert P(ops.connected_components) == dict(values=inspect._empty, level=inspect._empty, invert=False, connectivity=14)
    kc = P(ops.keep_components)
    assert (kc["largest"], kc["min_size"], kc["fill"], kc["invert"], kc["connectivity"], kc["return_labels"]) == (True, 0, None, False, 14, False)
    em = P(extract_shapes.extract_mesh)
    assert (em["keep_largest"], em["min_component"]) == (False, 0)


def test_extract_mesh_tsdf_takes_its_keywords_out_of_render_kwargs(monkeypatch):
    """Its parameter list is pinned (tests/test_tsdf_cpu.py), so hidden_min, keep_largest, min_component and fill_cavities arrive among
    render_kwargs.  With the pieces around it replaced by recorders: none of the four reaches the generator, hidden_min reaches
    tsdf_volume, the filters run in the stated order with the stated fills on the volume that the isosurface then reads, and with the
    defaults no filter runs at all."""
    import cnerf_amd
    from cnerf_amd import extract_shapes, ops, views
    doc = extract_shapes.extract_mesh_tsdf.__doc__
    assert all(w in doc for w in ("hidden_min=1", "keep_largest=False", "min_component=0", "fill_cavities=False"))
    calls = []

    def render_views(gen, z, cams, R, fov, r0, r1, S, per_batch, **kw):
        calls.append(("render", kw))
        return "pixels", "depth"

    def tsdf_volume(pixels, depth, cams, fov, r0, r1, **kw):
        calls.append(("volume", kw["hidden_min"]))
        return "tsdf0", None, "rgb", (0.0, 0.0, 0.0), 0.5

    def keep_components(values, level, **kw):
        calls.append(("keep", values, level, kw))
        return values + "+"

    def isosurface(values, level, **kw):
        calls.append(("iso", values, level))
        return "mesh"

    monkeypatch.setattr(views, "render_views", render_views)
    monkeypatch.setattr(views, "tsdf_volume", tsdf_volume)
    monkeypatch.setattr(ops, "keep_components", keep_components)
    monkeypatch.setattr(ops, "isosurface", isosurface)
    args = (None, None, None, 8, 30.0, 0.5, 2.5, 12)
    assert extract_shapes.extract_mesh_tsdf(*args, clamp_mode="relu") == "mesh"
    assert calls == [("render", dict(clamp_mode="relu")), ("volume", 1), ("iso", "tsdf0", 0.0)]
    del calls[:]
    extract_shapes.extract_mesh_tsdf(*args, clamp_mode="relu", hidden_min=0, keep_largest=True, min_component=7, fill_cavities=True)
    assert calls == [("render", dict(clamp_mode="relu")), ("volume", 0),
                     ("keep", "tsdf0", 0.0, dict(largest=True, min_size=7, fill=-1.0)),
                     ("keep", "tsdf0+", 0.0, dict(largest=True, fill=1.0, invert=True)), ("iso", "tsdf0++", 0.0)]
    del calls[:]
    extract_shapes.extract_mesh_tsdf(*args, min_component=3)
    assert calls[2] == ("keep", "tsdf0", 0.0, dict(largest=False, min_size=3, fill=-1.0)) and calls[3] == ("iso", "tsdf0+", 0.0)


def test_refusals_come_before_any_launch_in_the_stated_order(L):
    """CNERF_EINVAL with a message, nothing launched: there is no GPU here and the device pointers are made up.  The order is shape,
    NULLs, level, connectivity, invert / largest_only, min_size, fill: a call that is wrong in two ways is refused for the earlier one."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    nb = ctypes.c_size_t()

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def label(shape=(8, 8, 8), values=fake, level=0.0, invert=0, conn=14, labels=fake, sizes=fake, stats=fake, ws=fake):
        return lib.cnerf_components_label(*shape, values, level, invert, conn, labels, sizes, stats, ws, None)

    def filt(shape=(8, 8, 8), values=fake, labels=fake, sizes=fake, stats=fake, largest=1, min_size=0, fill=-1.0, out=fake):
        return lib.cnerf_components_filter(*shape, values, labels, sizes, stats, largest, min_size, fill, out, None)

    nan, inf = float("nan"), float("inf")
    for shape, word in (((1, 8, 8), "n0=1"), ((8, 0, 8), "n1=0"), ((8, 8, 1025), "n2=1025"), ((-3, 8, 8), "n0=-3"), ((1024, 1024, 256), "2^27")):
        refused(lib.cnerf_components_bytes(*shape, ctypes.byref(nb)), word)
        refused(label(shape=shape, values=None, level=nan, conn=26, invert=2), word)             # the shape before everything else
        refused(filt(shape=shape, out=None, largest=2, min_size=-1, fill=nan), word)
    assert lib.cnerf_components_bytes(1024, 1024, 128, ctypes.byref(nb)) == 0                    # exactly 2^27 points
    for name in ("values", "labels", "sizes", "stats", "ws"):
        refused(label(**{name: None}, level=nan, conn=26, invert=2), "NULL")                     # NULLs before level, connectivity, invert
    for name in ("values", "labels", "sizes", "stats", "out"):
        refused(filt(**{name: None}, largest=2, min_size=-1, fill=nan), "NULL")
    for bad in (nan, inf, -inf):
        refused(label(level=bad, conn=26, invert=2), "level")                                    # level before connectivity and invert
    for conn in (0, 4, 8, 18, 26, -6):
        refused(label(conn=conn, invert=2), "connectivity")                                      # connectivity before invert
    for bad in (2, -1):
        refused(label(invert=bad), "invert")
        refused(filt(largest=bad, min_size=-1, fill=nan), "largest_only")                        # largest_only before min_size and fill
    refused(filt(min_size=-1, fill=nan), "min_size")                                             # min_size before fill
    refused(filt(fill=nan), "fill")
    refused(label(ws=ctypes.c_void_p(0x1004)), "aligned")                                        # after all of the above
