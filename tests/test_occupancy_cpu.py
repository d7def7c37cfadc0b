"""Occupancy grids (cnerf_occupancy_*, cnerf_render_rays_masked_forward), no GPU: the host code's exports, workspace sizes and
refusals, and the NumPy statement of the semantics (tests/occupancy_common.py) on hand-made points and grids.

The refusal of a stream that is being captured needs a stream, hence a GPU: tests/test_gpu_occupancy.py has it."""
import ctypes

import numpy as np
import pytest

import occupancy_common as OC

ENTRIES = ("cnerf_occupancy_build", "cnerf_occupancy_compact_bytes", "cnerf_occupancy_compact", "cnerf_occupancy_expand",
           "cnerf_render_rays_masked_workspace_bytes", "cnerf_render_rays_masked_forward")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    import cnerf_amd
    return cnerf_amd._lib


def rays_cfg(L, B=2, S=12, hierarchical=True):
    cfg = L.Cfg()
    cfg.B, cfg.S, cfg.V, cfg.C, cfg.H, cfg.L = B, S, 8, 32, 64, 4
    for i in range(4):
        cfg.layer_kind[i] = L.LAYER_FILM
    cfg.voxel_length, cfg.ray_start, cfg.ray_end = 1.2, 0.25, 1.95
    cfg.n_levels, cfg.level_V[0], cfg.level_C[0] = 1, 8, 32
    cfg.precision = L.PREC_FP32
    cfg.flags = L.F_HIERARCHICAL if hierarchical else 0
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
    assert [f for f, _ in L.Occupancy._fields_] == ["bits", "G", "lo", "side"] and ctypes.sizeof(L.Occupancy) == 32
    assert "typedef struct cnerf_occupancy" in header


def test_workspace_sizes_are_positive_and_grow_with_n(L):
    lib = L.lib()
    n = ctypes.c_size_t()
    sizes = []
    for pts in (1, 2048, 2049, 1 << 20, 1 << 26):
        assert lib.cnerf_occupancy_compact_bytes(2, pts, ctypes.byref(n)) == 0, lib.cnerf_last_error()
        sizes.append(n.value)
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 2 * ((1 << 26) // 2048) * 4                # a count per 2048 points and image
    plain, masked = [], []
    for P in (1, 37, 100, 1 << 14):
        assert lib.cnerf_render_rays_workspace_bytes(ctypes.byref(rays_cfg(L)), P, ctypes.byref(n)) == 0
        plain.append(n.value)
        assert lib.cnerf_render_rays_masked_workspace_bytes(ctypes.byref(rays_cfg(L)), P, ctypes.byref(n)) == 0, lib.cnerf_last_error()
        masked.append(n.value)
    assert masked[0] > 0 and all(a < b for a, b in zip(masked, masked[1:]))
    # the unmasked call's buffers, then live positions (3), values (4) and ranks (1) of one pass
    assert all(m >= p + 2 * P * 12 * 8 * 4 for m, p, P in zip(masked, plain, (1, 37, 100, 1 << 14)))


def test_refusals_come_before_any_launch(L):
    """Each returns CNERF_EINVAL with a message; nothing was launched: there is no GPU here, the device pointers are made up."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    rays = L.Rays()
    rays.origins = rays.dirs = 0x1000
    vols = L.Volumes()
    vols.level[0] = 0x1000
    rng = L.Rng()
    rng.u_fine = 0x1000

    def refused(rc, *words):
        msg = lib.cnerf_last_error().decode()
        assert rc == -22 and msg and all(w in msg for w in words), (rc, msg)

    def masked(cfg, oc, P=10, r=rays):
        return lib.cnerf_render_rays_masked_forward(ctypes.byref(cfg), ctypes.byref(r), P, ctypes.byref(oc) if oc is not None else None, ctypes.byref(vols),
                                                    fake, fake, fake, ctypes.byref(rng), fake, fake, None, None, fake, None)

    def compact(oc, B=2, n=100):
        return lib.cnerf_occupancy_compact(ctypes.byref(oc) if oc is not None else None, B, n, fake, fake, fake, fake, fake, None)

    for call in (lambda oc: masked(rays_cfg(L), oc), compact):
        refused(call(None), "occupancy is NULL")
        for G in (0, 3, 6, 10, 260, -4):
            refused(call(occupancy(L, G=G)), f"G={G}")
        for side in (0.0, -2.0, float("nan"), float("inf")):
            refused(call(occupancy(L, side=side)), "side")
        refused(call(occupancy(L, bits=None)), "bits is NULL")
    cfg = rays_cfg(L)
    cfg.drop_p = 0.25
    refused(masked(cfg, occupancy(L)), "dropout")
    # what the unmasked entry refuses, too
    refused(masked(rays_cfg(L, S=1), occupancy(L)), "S=1")
    refused(masked(rays_cfg(L), occupancy(L), P=0), "rays_per_image")
    no_origins = L.Rays()
    no_origins.dirs = 0x1000
    refused(masked(rays_cfg(L), occupancy(L), r=no_origins), "origins")
    n = ctypes.c_size_t()
    refused(lib.cnerf_render_rays_masked_workspace_bytes(ctypes.byref(cfg), 10, ctypes.byref(n)), "dropout")
    refused(lib.cnerf_render_rays_masked_workspace_bytes(ctypes.byref(rays_cfg(L)), 1 << 28, ctypes.byref(n)), "n_per_image")      # 2^28 * 12 points
    # the stages
    refused(compact(occupancy(L), n=0), "n_per_image")
    refused(compact(occupancy(L), n=1 << 31), "n_per_image")
    refused(compact(occupancy(L), B=0), "B=0")
    refused(lib.cnerf_occupancy_compact(ctypes.byref(occupancy(L)), 2, 100, None, fake, fake, fake, fake, None), "NULL")
    refused(lib.cnerf_occupancy_compact_bytes(2, 0, ctypes.byref(n)), "n_per_image")
    for G in (0, 5, 300):
        refused(lib.cnerf_occupancy_build(2, G, 1, 0.0, fake, fake, None), f"G={G}")
    for d in (-1, 5):
        refused(lib.cnerf_occupancy_build(2, 8, d, 0.0, fake, fake, None), f"dilate={d}")
    refused(lib.cnerf_occupancy_build(2, 8, 1, 0.0, None, fake, None), "NULL")
    refused(lib.cnerf_occupancy_build(2, 8, 1, 0.0, fake, ctypes.c_void_p(0x1004), None), "aligned")
    refused(lib.cnerf_occupancy_expand(2, 0, fake, fake, ctypes.c_void_p(0x2000), None), "n_per_image")
    refused(lib.cnerf_occupancy_expand(2, 10, fake, fake, fake, None), "distinct")
    refused(lib.cnerf_occupancy_expand(2, 10, fake, ctypes.c_void_p(0x1004), ctypes.c_void_p(0x2000), None), "aligned")
    refused(lib.cnerf_occupancy_expand(2, 10, None, fake, ctypes.c_void_p(0x2000), None), "NULL")


# ---------------------------------------------------------------------------------------------------------------------
# the NumPy statement itself, on hand-made points
# ---------------------------------------------------------------------------------------------------------------------
def test_inside_and_cell_on_hand_made_points():
    G, lo, side = 8, -1.0, 2.0
    f = np.float32
    inside = lambda p: bool(OC.inside(np.array([p], f), [lo] * 3, side, G)[0])
    cell = lambda p: int(OC.cell_index(np.array([p], f), [lo] * 3, side, G)[0])
    assert inside([-1, -1, -1]) and cell([-1, -1, -1]) == 0                      # exactly lo: cell 0
    assert not inside([1, 0, 0]) and not inside([1, 1, 1]) and cell([1, 0, 0]) == -1      # exactly lo + side: outside
    assert inside([0.99, 0, 0]) and cell([0.99, 0, 0]) == (7 * G + 4) * G + 4
    assert not inside([np.nextafter(f(1), f(0)), 0, 0])        # p - lo is rounded first: 2 - 2^-24 is a tie and rounds to 2 = side
    assert not inside([np.nextafter(f(-1), f(-2)), 0, 0])
    for k in range(G):                                                            # a cell edge belongs to the cell above it
        x = f(lo + k * side / G)
        assert cell([x, -1, -1]) == k * G * G and cell([-1, x, -1]) == k * G and cell([-1, -1, x]) == k
    assert cell([-0.0, 0.0, 1e-42]) == (4 * G + 4) * G + 4                        # -0.0 and a denormal: the cell of 0
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = [0.0, 0.0, 0.0]
            p[axis] = bad
            assert not inside(p) and cell(p) == -1
    # a box at the origin: -0.0 is inside (t = -0.0 >= 0), cell 0; a negative denormal is not (no flush to zero in this statement)
    at0 = lambda p: int(OC.cell_index(np.array([p], f), [0.0] * 3, side, G)[0])
    assert at0([-0.0, -0.0, 0.0]) == 0 and at0([1e-42, 0, 0]) == 0 and at0([-1e-42, 0, 0]) == -1
    # every operation rounded on its own: a box whose inv is not a power of two
    G3, lo3, side3 = 12, f(0.1), f(0.7)
    pts = np.random.default_rng(0).uniform(0.0, 0.9, (1000, 3)).astype(f)
    t = ((pts - lo3).astype(f) * f(f(G3) / side3)).astype(f)
    want = np.where(((t >= 0) & (t < G3)).all(1), (np.floor(t[:, 0]) * G3 + np.floor(t[:, 1])) * G3 + np.floor(t[:, 2]), -1).astype(np.int64)
    assert np.array_equal(OC.cell_index(pts, [lo3] * 3, side3, G3), want) and (want >= 0).sum() > 100 and (want < 0).sum() > 100


def test_live_edge_points_and_compaction():
    G, lo, side = 8, -1.0, 2.0
    pts = OC.edge_points(lo, side, G)
    ins = OC.inside(pts, [lo] * 3, side, G)
    assert ins[0] and not ins[1] and not ins[2] and ins[3:3 + G].all() and not ins[3 + G]           # lo, lo + side, the edges k = 0..G
    assert ins[-7] and not ins[-6] and not ins[-5] and not ins[-4] and not ins[-3] and ins[-2] and ins[-1]
    clear, full = np.zeros(G ** 3 // 32, np.uint32), np.full(G ** 3 // 32, 0xFFFFFFFF, np.uint32)
    assert np.array_equal(OC.live(pts, clear, [lo] * 3, side, G), ~ins)           # outside the box nothing is skipped
    assert OC.live(pts, full, [lo] * 3, side, G).all()
    one = clear.copy()
    idx = (5 * G + 4) * G + 4                                                      # the cell of (0.25 .. 0.5, 0 .. 0.25, 0 .. 0.25)
    one[idx >> 5] |= np.uint32(1) << np.uint32(idx & 31)
    probe = np.array([[0.3, 0.1, 0.1], [0.3, 0.1, 0.3], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [2.0, 0.1, 0.1]], np.float32)
    assert OC.live(probe, one, [lo] * 3, side, G).tolist() == [True, False, True, False, True]
    rank, counts, lv = OC.compact(np.stack([probe, probe]), np.stack([one, clear]), [lo] * 3, side, G)
    assert rank.tolist() == [[0, -1, 1, -1, 2], [-1, -1, -1, -1, 0]] and counts.tolist() == [3, 1]
    vals = np.arange(2 * 5 * 4, dtype=np.float32).reshape(2, 5, 4)
    out = OC.expand(rank, vals)
    assert OC.same_bits(out[0, 0], vals[0, 0]) and OC.same_bits(out[0, 2], vals[0, 1]) and OC.same_bits(out[0, 4], vals[0, 2])
    assert OC.same_bits(out[0, 1], OC.FILL) and OC.same_bits(out[1, 4], vals[1, 0]) and np.isneginf(out[1, :4, 3]).all()


def test_bit_build_on_hand_made_grids():
    G = 4
    s = np.full((1, G + 1, G + 1, G + 1), -1.0, np.float32)
    s[0, 2, 2, 2] = 1.0                                   # one corner above the threshold: the 8 cells around it
    cells = OC.build_cells(s.reshape(1, -1), G, 0.0, 0).reshape(G, G, G)
    assert cells.sum() == 8 and cells[1:3, 1:3, 1:3].all()
    assert OC.build_cells(s.reshape(1, -1), G, 0.0, 1).all()                      # cells 0..3 on every axis
    assert not OC.build_cells(s.reshape(1, -1), G, 1.0, 2).any()                  # equal to the threshold: not set
    s[0, 2, 2, 2] = -1.0
    s[0, 0, 0, 4] = np.nan                                # a NaN corner sets the one cell that owns it, and its neighbours when dilated
    cells = OC.build_cells(s.reshape(1, -1), G, 0.0, 0).reshape(G, G, G)
    assert cells.sum() == 1 and cells[0, 0, 3]
    cells = OC.build_cells(s.reshape(1, -1), G, 0.0, 1).reshape(G, G, G)
    assert cells.sum() == 8 and cells[:2, :2, 2:].all()
    s[0, 0, 0, 4] = -np.inf
    s[0, 4, 4, 4] = np.inf
    cells = OC.build_cells(s.reshape(1, -1), G, 1e30, 0).reshape(G, G, G)
    assert cells.sum() == 1 and cells[3, 3, 3]
    # bit order: cell (ix, iy, iz) is bit (ix G + iy) G + iz of word idx >> 5
    words = OC.build_bits(s.reshape(1, -1), G, 1e30, 0)
    assert words.shape == (1, 2) and words.dtype == np.uint32 and words[0].tolist() == [0, 1 << 31]
    c = np.zeros(64, bool)
    c[[0, 33]] = True
    assert OC.pack_bits(c).tolist() == [1, 2] and OC.bit_at(OC.pack_bits(c), np.arange(64)).tolist() == c.tolist()
    assert 0.05 < OC.ball_cells(8, 2.5).mean() < 0.25 and OC.ball_cells(8, 8).all()
