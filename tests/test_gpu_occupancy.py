"""Occupancy grids on the GPU: cnerf_occupancy_build / _compact / _expand against their NumPy statement (tests/occupancy_common.py),
cnerf_render_rays_masked_forward against the unmasked cnerf_render_rays_forward, and the public interface
(ImplicitGenerator3d.build_occupancy, render_rays(..., occupancy=grid)).

Shapes: B = 2 with a different bit set per image; G in {4, 8, 12} for the build, 8 for the compaction and the renders, 32 for the
truthful mask; point counts on both sides of a wave (32 / 64 would be the same path: 31, 32, 33), of a 256-thread round (255, 256, 257),
several 2048-point chunks (5000), a second chunk of a full wave and a wave of one lane whose first chunk has a round without a live
point before a round of nothing else (2048 + 65: what the two LDS slots of the rank kernel are for) and more chunks than one round of
the chunk scan holds (257 chunks: 2048 * 256 + 5); renders of 2 x 37 rays with 12 (+ 12) or 10 samples, so that no count is a multiple
of the 32-point tile.

Gates: every stage and every rgb_sigma bit for bit.  pixels / dist of a masked render against the oracle's merge + composite in float64 on
the device's own masked rgb_sigma and depths: COMPOSITE_TOL = 1e-5, the gate of tests/test_gpu_ray_stages.py::test_composite_vs_float64
(a literal there, so it cannot be imported; that test measured 1.5e-6 at most on an MI355X)."""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_common as OC
import render_rays_common as RC
from conftest import scaled_err
from oracle import render_oracle as O

pytestmark = pytest.mark.gpu

LO, SIDE = -1.0, 2.0
BOX = ([LO] * 3, SIDE)
COMPOSITE_TOL = 1e-5
CANARY = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a GPU"
    return torch.device("cuda:0")


def words_to_device(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)


def grid_of(words, dev, G):
    from cnerf_amd import ops
    return ops.OccupancyGrid(words_to_device(words, dev), (LO, LO, LO), SIDE, G)


def mask_words(kind, G, seed):
    if kind == "set":
        return np.full(G ** 3 // 32, 0xFFFFFFFF, np.uint32)
    if kind == "clear":
        return np.zeros(G ** 3 // 32, np.uint32)
    cells = np.random.default_rng(seed).random(G ** 3) < 0.5
    if kind == "rounds":                                                      # the first cell clear, the last one set
        cells[0], cells[-1] = False, True
    return OC.pack_bits(cells)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the bits
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("G", [4, 8, 12])
def test_build_equals_numpy_word_for_word(dev, G, dilate):
    """sigma ~ N(0,1) at the corners, threshold 1.3 (about half the cells set without dilation); planted: a NaN, +inf, -inf, and a block
    of corners at -5 whose centre is exactly the threshold -- the cells that see only that block stay clear at dilate 0."""
    from cnerf_amd import ops
    B, thr = 2, 1.3
    rng = np.random.default_rng(100 * G + dilate)
    s = rng.standard_normal((B, G + 1, G + 1, G + 1)).astype(np.float32)
    s[:, 0:3, 0:3, 0:3] = -5.0
    s[:, 1, 1, 1] = np.float32(thr)
    s[0, G, G, 2] = np.nan
    s[1, 2, G, G] = np.inf
    s[1, G, 0, G // 2] = -np.inf
    s[0, G // 2 + 1, G // 2 + 1, G // 2 + 1] = np.nan
    want = OC.build_bits(s.reshape(B, -1), G, thr, dilate)
    cells = OC.build_cells(s.reshape(B, -1), G, thr, dilate).reshape(B, G, G, G)
    assert cells[0, G - 1, G - 1, 1] and cells[0, G - 1, G - 1, 2] and cells[1, 1, G - 1, G - 1]            # NaN and +inf set their cells
    if dilate == 0:
        assert not cells[:, 0:2, 0:2, 0:2].any()                                                         # max == threshold: clear
    assert 0.05 < cells.mean() <= 1.0
    got = ops.occupancy_build(torch.from_numpy(s.reshape(B, -1)).to(dev), G, thr, dilate)
    assert got.dtype == torch.int32 and got.shape == (B, G ** 3 // 32)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    if dilate == 2 and G == 4:
        assert cells.all()                                                                               # the window is the whole grid


# ---------------------------------------------------------------------------------------------------------------------
# 2. compaction and expansion
# ---------------------------------------------------------------------------------------------------------------------
ROUNDS_N = 2048 + 65


def compaction_points(B, n, G, seed):
    """Uniform over 1.3 x the box; the hand-made edge points replace the first rows (as many as fit).  n = ROUNDS_N: the first 256
    rows of image 1 (round 0 of its first chunk) sit in the first cell, the next 256 (round 1) in the last."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(1.3 * LO, 1.3 * (LO + SIDE), (B, n, 3)).astype(np.float32)
    edge = OC.edge_points(LO, SIDE, G)
    k = min(n, len(edge))
    pts[0, :k] = edge[:k]
    pts[1, n - k:] = edge[len(edge) - k:]
    if n == ROUNDS_N:
        pts[1, :256] = LO + 0.5 * SIDE / G
        pts[1, 256:512] = LO + SIDE - 0.5 * SIDE / G
    return pts


@pytest.mark.parametrize("n", [1, 31, 32, 33, 255, 256, 257, ROUNDS_N, 5000, 2048 * 256 + 5])
def test_compaction_equals_numpy(dev, n):
    from cnerf_amd import ops
    B, G = 2, 8
    pts = compaction_points(B, n, G, n)
    d_pts = torch.from_numpy(pts).to(dev)
    for kinds in (("set", "random"), ("clear", "random"), ("random", "clear")) + ((("random", "rounds"),) if n == ROUNDS_N else ()):
        words = np.stack([mask_words(k, G, 7 * n + i) for i, k in enumerate(kinds)])
        rank, counts, lv = OC.compact(pts, words, *BOX, G)
        if "rounds" in kinds:
            assert not lv[1, :256].any() and lv[1, 256:512].all()              # a round of 256 without a live point, then one of nothing else
        if n >= 5000:
            assert 0.3 < lv[kinds.index("random")].mean() < 0.9                # inside and skipped, inside and kept, outside
        pad = 64
        flat_live = torch.full((B * n * 3 + pad,), CANARY, device=dev)
        flat_rank = torch.full((B * n + pad,), 777, dtype=torch.int32, device=dev)
        g_rank, g_live, g_counts = ops.occupancy_compact(grid_of(words, dev, G), d_pts, rank=flat_rank[:B * n].view(B, n),
                                                         live_points=flat_live[:B * n * 3].view(B, n, 3))
        assert np.array_equal(g_counts.cpu().numpy(), counts), (kinds, g_counts.cpu().numpy(), counts)
        assert np.array_equal(g_rank.cpu().numpy(), rank), kinds
        g_live = g_live.cpu().numpy()
        for b in range(B):
            assert OC.same_bits(g_live[b, :counts[b]], pts[b][lv[b]]), (kinds, b)
            assert (g_live[b, counts[b]:] == CANARY).all(), (kinds, b)        # rows behind counts[b] are untouched
        assert (flat_live[B * n * 3:] == CANARY).all().item() and (flat_rank[B * n:] == 777).all().item()


@pytest.mark.parametrize("n", [1, 33, 257, 5000])
def test_expansion_is_exact(dev, n):
    from cnerf_amd import ops
    B = 2
    rng = np.random.default_rng(n)
    lv = rng.random((B, n)) < 0.5
    lv[1] = rng.random(n) < 0.1
    rank = np.where(lv, np.cumsum(lv, 1) - 1, -1).astype(np.int32)
    vals = rng.standard_normal((B, n, 4)).astype(np.float32)
    vals[0, 0] = [np.nan, -0.0, np.inf, -np.inf]                              # whatever the field wrote travels as bits
    want = OC.expand(rank, vals)
    pad = 64
    flat = torch.full((B * n * 4 + pad,), CANARY, device=dev)
    out = ops.occupancy_expand(torch.from_numpy(rank).to(dev), torch.from_numpy(vals).to(dev), out=flat[:B * n * 4].view(B, n, 4))
    assert OC.same_bits(out.cpu().numpy(), want)
    assert np.isneginf(want[~lv][:, 3]).all() and (want[~lv][:, :3] == 0).all()
    assert (flat[B * n * 4:] == CANARY).all().item()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the masked render against the unmasked one
# ---------------------------------------------------------------------------------------------------------------------
def on_device(case, dev):
    case.gen.to(dev)
    case.gen.set_device(dev)
    case.gen.eval()


def render(case, dev, rng, occupancy=None):
    """gen.render_rays under no_grad -> (pixels, dist, aux), NumPy / CPU."""
    T = lambda t: None if t is None else t.to(dev)
    aux = {}
    kw = {} if occupancy is None else {"occupancy": occupancy}
    with torch.no_grad():
        px, dist = case.gen.render_rays(RC.generator_z(case, [T(v) for v in case.vols], T(case.glob)), T(case.origins), T(case.dirs), RC.RAY_START, RC.RAY_END,
                                        case.S, case.hierarchical, clamp_mode=case.clamp, nerf_noise=case.noise, white_back=case.white_back,
                                        last_back=case.last_back, _rng={k: T(v) for k, v in rng.items()}, _aux=aux, **kw)
    return px.cpu().numpy(), dist.cpu().numpy(), {k: v.cpu().numpy() for k, v in aux.items()}


def forced_depths(case, dev):
    """Fine depths to force on both renders (masking changes the coarse weights, hence the resampled depths): the unmasked render's."""
    if not case.hierarchical:
        return dict(case.rng)
    return dict(case.rng, fine_z=torch.from_numpy(render(case, dev, case.rng)[2]["fine_z"]))


def numpy_live(aux, key, words, G):
    pts = aux[key]
    B = pts.shape[0]
    return np.stack([OC.live(pts[b].reshape(-1, 3), words[b], *BOX, G) for b in range(B)])


def check_pass(name, masked, plain, words, G):
    """rgb_sigma of a pass: the unmasked values bit for bit where NumPy says live, the fill elsewhere; the live count."""
    assert np.array_equal(masked[name + "_points"], plain[name + "_points"])
    lv = numpy_live(plain, name + "_points", words, G)
    B = lv.shape[0]
    want = np.where(lv[..., None], plain[name + "_rgb_sigma"].reshape(B, -1, 4), OC.FILL)
    assert OC.same_bits(masked[name + "_rgb_sigma"].reshape(B, -1, 4), want), name
    assert np.array_equal(masked["live_" + name], lv.sum(1)), (name, masked["live_" + name], lv.sum(1))
    return lv


def oracle_image(case, aux, rng):
    """merge + composite of the oracle in float64 on the device's rgb_sigma and depths -> pixels (B,P,3), dist (B,P)."""
    D = lambda a: torch.from_numpy(np.asarray(a)).double()
    keep = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        if case.hierarchical:
            out, z, _ = O.merge_by_depth(D(aux["fine_rgb_sigma"]), D(aux["coarse_rgb_sigma"]), D(rng["fine_z"].reshape(case.B, case.P, case.S)),
                                         D(aux["coarse_z"]))
        else:
            out, z = D(aux["coarse_rgb_sigma"]), D(aux["coarse_z"])
        eps = rng.get("eps_final") if case.noise else None
        rgb, dist, _ = O.composite(out, z, None if eps is None else eps.reshape(case.B, case.P, -1).double(), case.noise, case.clamp, case.white_back,
                                   case.last_back)
    finally:
        torch.set_default_dtype(keep)
    return (rgb * 2 - 1).numpy(), dist.numpy()


CONFIGS = {"hier_softplus_noise": dict(S=12, hierarchical=True, clamp="softplus", noise=0.3),
           "flat_relu": dict(S=10, hierarchical=False, clamp="relu", noise=0.0)}
VARIANTS = {"SHORTSIREN_FG": ("fp32", "fp16x3", "fp16"), "SHORTSIREN": ("fp32",), "TALLSIREN": ("fp32",), "SHORTSIREN_FG_Pyrmd": ("fp32",)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_masked_render_against_the_unmasked_one(dev, variant, config):
    c = CONFIGS[config]
    G = 8
    case = RC.make_case(variant, 64, 2, 37, c["S"], V=8, seed=5, hierarchical=c["hierarchical"], clamp=c["clamp"], noise=c["noise"])
    on_device(case, dev)
    words = np.stack([mask_words("random", G, 11), mask_words("random", G, 12)])
    grid = grid_of(words, dev, G)
    for prec in VARIANTS[variant]:
        case.gen.siren.precision = prec
        rng = forced_depths(case, dev)
        _, _, plain = render(case, dev, rng)
        px, dist, masked = render(case, dev, rng, grid)
        lv = check_pass("coarse", masked, plain, words, G)
        share = [lv.mean()]
        if case.hierarchical:
            share.append(check_pass("fine", masked, plain, words, G).mean())
        assert all(0.2 < s < 0.95 for s in share), share                   # both kinds of sample in every pass
        want_px, want_dist = oracle_image(case, masked, rng)
        e_p, e_d = scaled_err(px, want_px), scaled_err(dist, want_dist)
        print(f"{variant} {config} [{prec}]: live share {share}; pixels {e_p:.2e} dist {e_d:.2e} vs float64 merge + composite")
        assert np.isfinite(px).all() and np.isfinite(dist).all()
        assert e_p < COMPOSITE_TOL and e_d < COMPOSITE_TOL, (prec, e_p, e_d)


def test_an_image_without_a_live_point_is_the_background(dev):
    """Image 0: all-clear bits and every sample inside the box -> no field launch for it, pixels = 1 (white_back), dist = 0; image 1
    (all-set bits) is what the unmasked render gives."""
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 12, V=8, seed=9, clamp="relu", noise=0.0)
    g = torch.Generator().manual_seed(1)
    case.origins = (torch.rand(2, 37, 3, generator=g) * 0.4 - 0.2).contiguous()
    d = torch.randn(2, 37, 3, generator=g)
    case.dirs = (d / d.norm(dim=-1, keepdim=True) * 0.35).contiguous()          # |o| + 2.03 |d| < 1: inside the box on every axis
    on_device(case, dev)
    words = np.stack([mask_words("clear", 8, 0), mask_words("set", 8, 0)])
    px0, dist0, plain = render(case, dev, case.rng)
    px, dist, aux = render(case, dev, case.rng, grid_of(words, dev, 8))
    assert OC.inside(aux["coarse_points"], *BOX, 8).all() and OC.inside(aux["fine_points"], *BOX, 8).all()
    assert aux["live_coarse"].tolist() == [0, 37 * 12] and aux["live_fine"].tolist() == [0, 37 * 12]
    assert (px[0] == 1.0).all() and (dist[0] == 0.0).all()
    assert np.isneginf(aux["coarse_rgb_sigma"][0, ..., 3]).all() and np.isneginf(aux["fine_rgb_sigma"][0, ..., 3]).all()
    assert OC.same_bits(px[1], px0[1]) and OC.same_bits(dist[1], dist0[1])
    assert OC.same_bits(aux["fine_rgb_sigma"][1], plain["fine_rgb_sigma"][1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. a truthful mask changes nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,S,hier", [("SHORTSIREN_FG", 12, True), ("SHORTSIREN", 12, True), ("TALLSIREN", 10, False)])
def test_truthful_mask_renders_the_same_image(dev, variant, S, hier):
    """relu, no noise: the bit of every cell that holds a coarse or fine sample of density > 0 in the unmasked render is set (G = 32), every
    other bit clear.  A skipped sample had density <= 0, hence weight 0 and no effect on the transmittance: pixels and dist of the masked
    render are the unmasked ones bit for bit.  At least 20 % of all samples must be skipped for this to show anything; the CPU oracle on
    these cases skips 38 % (SHORTSIREN_FG), 63 % (SHORTSIREN) and 26 % (TALLSIREN)."""
    G = 32
    case = RC.make_case(variant, 64, 2, 37, S, V=8, seed=3, hierarchical=hier, clamp="relu", noise=0.0)
    on_device(case, dev)
    px0, dist0, plain = render(case, dev, case.rng)
    cells = np.zeros((case.B, G ** 3), bool)
    for name in ("coarse", "fine") if hier else ("coarse",):
        pts, sig = plain[name + "_points"].reshape(case.B, -1, 3), plain[name + "_rgb_sigma"].reshape(case.B, -1, 4)[..., 3]
        for b in range(case.B):
            idx = OC.cell_index(pts[b], *BOX, G)
            cells[b, idx[(idx >= 0) & (sig[b] > 0)]] = True
    px, dist, aux = render(case, dev, case.rng, grid_of(OC.pack_bits(cells), dev, G))
    total = case.B * case.P * S * (2 if hier else 1)
    evaluated = int(aux["live_coarse"].sum()) + (int(aux["live_fine"].sum()) if hier else 0)
    skipped = 1.0 - evaluated / total
    print(f"{variant}: {skipped * 100:.1f} % of {total} samples skipped")
    assert OC.same_bits(px, px0) and OC.same_bits(dist, dist0)
    assert skipped >= 0.20, skipped


# ---------------------------------------------------------------------------------------------------------------------
# 5. the public interface, determinism, stream capture
# ---------------------------------------------------------------------------------------------------------------------
def test_generator_interface(dev):
    from cnerf_amd import ops
    G = 8
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 12, V=8, seed=21, clamp="relu", noise=0.0)
    on_device(case, dev)
    gen = case.gen
    z = (case.vols[0].to(dev), case.glob.to(dev))
    # build_occupancy: the NumPy build from gen.siren at the corner points lo + i (side / G); 729 corners in chunks of 200
    with torch.no_grad():
        grid = gen.build_occupancy(z, (LO, LO, LO), SIDE, resolution=G, threshold=0.0, dilate=1, max_points=200)
        ax = torch.tensor(LO, device=dev) + torch.arange(G + 1, device=dev, dtype=torch.float32) * (torch.tensor(SIDE, device=dev) / G)
        corners = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, -1, 3).expand(2, -1, -1).contiguous()
        sigma = gen.siren(corners, z)[..., 3].cpu().numpy()
    assert isinstance(grid, ops.OccupancyGrid) and (grid.G, grid.side, tuple(grid.lo)) == (G, SIDE, (LO, LO, LO))
    want = OC.build_bits(sigma, G, 0.0, 1)
    assert np.array_equal(grid.bits.cpu().numpy().view(np.uint32), want)
    print(f"build_occupancy: {OC.build_cells(sigma, G, 0.0, 1).mean() * 100:.0f} % of the cells set")
    # render_rays(..., occupancy=grid) is the ops call
    words = np.stack([mask_words("random", G, 31), mask_words("random", G, 32)])
    grid = grid_of(words, dev, G)
    px, dist, aux = render(case, dev, case.rng, grid)
    net = gen.siren
    o = dict(B=2, S=12, ray_start=RC.RAY_START, ray_end=RC.RAY_END, hier=True, clamp_mode="relu", noise_std=0.0, white_back=True, last_back=False)
    with torch.no_grad():
        freq, phase = net.film(z[1])
        rng = {k: v.to(dev) for k, v in case.rng.items()}
        o_px, o_dist, o_aux = ops.render_rays_forward(net, [ops.channel_last(z[0])], freq, phase, case.origins.to(dev), case.dirs.to(dev), o, rng,
                                                      want_aux=True, occupancy=grid)
    assert OC.same_bits(px, o_px.cpu().numpy()) and OC.same_bits(dist, o_dist.cpu().numpy())
    assert np.array_equal(aux["live_coarse"], o_aux["live_coarse"].numpy()) and np.array_equal(aux["live_fine"], o_aux["live_fine"].numpy())
    assert aux["live_coarse"].dtype == np.int32 and aux["live_coarse"].shape == (2,)
    # without `occupancy` the call is what it was: no live_* keys, and all-set bits give the same image bit for bit
    px0, dist0, plain = render(case, dev, case.rng)
    assert "live_coarse" not in plain
    full = grid_of(np.stack([mask_words("set", G, 0)] * 2), dev, G)
    px1, dist1, aux1 = render(case, dev, case.rng, full)
    assert OC.same_bits(px1, px0) and OC.same_bits(dist1, dist0) and aux1["live_coarse"].tolist() == [37 * 12] * 2
    assert OC.same_bits(aux1["coarse_rgb_sigma"], plain["coarse_rgb_sigma"]) and OC.same_bits(aux1["fine_rgb_sigma"], plain["fine_rgb_sigma"])
    # forward only; one grid per image
    args = (z, case.origins.to(dev), case.dirs.to(dev), RC.RAY_START, RC.RAY_END, 12, True)
    kw = dict(clamp_mode="relu", nerf_noise=0.0, white_back=True, _rng=rng)
    assert any(p.requires_grad for p in gen.parameters())
    with pytest.raises(RuntimeError, match="forward only"):
        gen.render_rays(*args, occupancy=grid, **kw)
    with torch.no_grad(), pytest.raises(ValueError, match="grids"):
        gen.render_rays(*args, occupancy=grid_of(words[:1], dev, G), **kw)
    with torch.no_grad(), pytest.raises(ops.L.CnerfError, match="int32"):
        gen.render_rays(*args, occupancy=ops.OccupancyGrid(grid.bits[:, :8].contiguous(), grid.lo, SIDE, G), **kw)


def test_masked_render_repeats_bit_for_bit(dev):
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 12, V=8, seed=5)
    on_device(case, dev)
    words = np.stack([mask_words("random", 8, 11), mask_words("random", 8, 12)])
    grid = grid_of(words, dev, 8)
    runs = [render(case, dev, case.rng, grid) for _ in range(5)]
    for px, dist, aux in runs[1:]:
        assert OC.same_bits(px, runs[0][0]) and OC.same_bits(dist, runs[0][1])
        for k in ("coarse_rgb_sigma", "fine_rgb_sigma", "fine_z"):
            assert OC.same_bits(aux[k], runs[0][2][k]), k
        assert np.array_equal(aux["live_coarse"], runs[0][2]["live_coarse"]) and np.array_equal(aux["live_fine"], runs[0][2]["live_fine"])


def test_a_capturing_stream_is_refused(dev):
    """cnerf_render_rays_masked_forward copies its live counts to the host and synchronises: on a stream that is being captured it
    returns CNERF_EINVAL before any launch (the captured graph stays empty); the same arguments render once the capture has ended."""
    import cnerf_amd
    from cnerf_amd import ops
    L = cnerf_amd._lib
    lib = L.lib()
    case = RC.make_case("SHORTSIREN_FG", 64, 2, 37, 10, V=8, seed=2, hierarchical=False, clamp="relu", noise=0.0)
    on_device(case, dev)
    net = case.gen.siren
    o = dict(B=2, S=10, ray_start=RC.RAY_START, ray_end=RC.RAY_END, hier=False, clamp_mode="relu", noise_std=0.0, white_back=True, last_back=False)
    with torch.no_grad():
        levels = [ops.channel_last(case.vols[0].to(dev))]
        freq, phase = net.film(case.glob.to(dev))
        cfg = ops._rays_cfg(net, o, levels)
        packed = ops.pack_field(net, cfg)
    nb = C.c_size_t()
    assert lib.cnerf_render_rays_masked_workspace_bytes(C.byref(cfg), 37, C.byref(nb)) == 0
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    org, drs = case.origins.to(dev), case.dirs.to(dev)
    rays = L.Rays()
    rays.origins, rays.dirs = org.data_ptr(), drs.data_ptr()
    vols = ops.volumes_struct(levels)
    bits = words_to_device(np.stack([mask_words("random", 8, 1), mask_words("random", 8, 2)]), dev)
    oc = L.Occupancy()
    oc.bits, oc.G, oc.side = bits.data_ptr(), 8, SIDE
    oc.lo[0] = oc.lo[1] = oc.lo[2] = LO
    pixels, dist = torch.zeros((2, 37, 3), device=dev), torch.zeros((2, 37), device=dev)
    live = (C.c_int32 * 4)(-1, -1, -1, -1)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(stream):
        rc = lib.cnerf_render_rays_masked_forward(C.byref(cfg), C.byref(rays), 37, C.byref(oc), C.byref(vols), p(packed), p(freq), p(phase), None, p(pixels),
                                                  p(dist), None, live, p(ws), C.c_void_p(stream.cuda_stream))
        return rc, lib.cnerf_last_error().decode()

    # the capture through the HIP runtime the library itself is linked against (dlsym on its handle reaches its dependencies)
    begin, end, destroy = lib.hipStreamBeginCapture, lib.hipStreamEndCapture, lib.hipGraphDestroy
    begin.argtypes, end.argtypes, destroy.argtypes = [C.c_void_p, C.c_int], [C.c_void_p, C.POINTER(C.c_void_p)], [C.c_void_p]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    handle, graph = C.c_void_p(side.cuda_stream), C.c_void_p()
    assert begin(handle, 1) == 0                          # hipStreamCaptureModeThreadLocal
    try:
        rc, msg = call(side)
    finally:
        assert end(handle, C.byref(graph)) == 0
        if graph.value:
            destroy(graph)
    assert rc == -22 and "captured" in msg, (rc, msg)
    assert list(live) == [-1] * 4 and not pixels.any().item()
    rc, msg = call(side)
    side.synchronize()
    assert rc == 0, msg
    assert all(0 < v <= 370 for v in live[:2]) and list(live[2:]) == [-1, -1] and torch.isfinite(pixels).all().item()
