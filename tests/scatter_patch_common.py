"""The patch scatter of the half-precision backward (cnerf_scatter_patches -> scatter_sorted_kernel, csrc/scatter_patch.hip) voxel by
voxel in float64: the expectation and its bound, a float32 NumPy restatement of the kernel's block decomposition, and the cases shared
by tests/test_scatter_patch_cpu.py (the decomposition's populations, an honest float32 emulation, the hazards) and
tests/test_gpu_scatter_patch.py (the kernel).

Expectation.  grad volume = base + float64 scatter of the rows gin with the float64 trilinear weights of the float32 sample positions:
scatter64 of tests/field_backward_stage_common.py with d g = 0 (the rows are inputs, not computed).  Its bound per voxel channel
    (3 + 2 k) u scatter(w |g|) + 3 DELTA scatter_nbr(|g|)
holds for ANY order of the voxel's k addends -- which is all the sorted kernel changes against a plain loop of atomics: run sums in a
register, runs split between half-waves, direct adds of the points outside the window or in a short tail.
One term is new because the entry ACCUMULATES and the test starts from a non-zero base b:  + k u |b|.  Each of the at most k adds a
voxel channel receives rounds a partial sum of magnitude <= |b| + sum |addend|: k u sum |addend| is inside the reordering term above
(which spends 2 k u where one order needs k - 1), the base's share is k u |b|.  k = 0 (no sample point's 4^3 neighbourhood holds the
voxel) leaves the bound at zero: the voxel must still hold its base bit for bit.  For this term k counts only the points whose row is
not zero: adding +-0 rounds nothing (the one-hot case).

Decomposition (scatter_patch.hip).  A block owns (image, 8 x 8-pixel patch (pr, pc), depth bin q), NQ = ceil(S / 4) bins.  Coarse pass:
bin q = samples 4 q .. 4 q + 3 of every ray of the patch, one round.  Fine pass: a sample belongs to the bin depth_bin() of its own
depth; the block walks the NQ quads of its rays in rounds, queues the samples of its bin (a ring of 512 slots) and processes 256 of
them whenever 256 wait; after the last round what is left goes as one batch, or straight to the volume when it is 48 points or fewer.
Inside a batch a point whose 8 corners lie inside the block's 8^3-voxel window is sorted by voxel and summed per run, every other point
is added directly.  float32 NumPy reproduces depth_bin() and the window origin operation for operation (the library is built with
-ffp-contract=off; the kernels' fmaf is emulated through float64).
"""
import math

import numpy as np

from field_backward_stage_common import F64, HALF_VOXEL, U, corners64, nbr_spread, scatter64      # (scatter64: corner_list's weights)

f32 = np.float32
BOX, PTS, DIRECT, RING = 8, 256, 48, 512        # SS_BOX, SS_PTS, SS_DIRECT, the queue's slots
FOV, RAY_START, RAY_END = 49.13, 0.25, 1.95


# ---- the expectation -------------------------------------------------------------------------------------------------------------------
def addend_count(points, V, npi_bound, live=None):
    """k of scatter64: per voxel the points whose 4^3 neighbourhood holds it (at most 8 per point of an image): (n_images, V, V, V, 1).
    live (n_images, npi) bool: the points that count (default: all)."""
    B, npi = points.shape[:2]
    i0 = corners64(points.reshape(-1, 3), V)[0]
    cell = np.zeros((B * V ** 3, 1))
    np.add.at(cell, (np.repeat(np.arange(B), npi) * V ** 3 + (i0[:, 2] * V + i0[:, 1]) * V + i0[:, 0], 0), 1.0 if live is None else live.reshape(-1) * 1.0)
    return np.minimum(nbr_spread(cell.reshape(B, V, V, V, 1)), 8.0 * npi_bound)


def expected(gin, points, tiles, base):
    """gin (feature tiles, n_images, npi, 32), points (n_images, npi, 3) float32, tiles [(level, first channel)] of the feature tiles,
    base [(n_images, V, V, V, C)] per level -> [(want, bound, k)] per level, float64."""
    npi = points.shape[1]
    out = []
    for lvl, b in enumerate(base):
        V = b.shape[1]
        want, bound = b.astype(F64), np.zeros(b.shape)
        k = addend_count(points, V, npi)
        for fi, (tl, cc) in enumerate(tiles):
            if tl != lvl:
                continue
            w_, b_ = scatter64(gin[fi], np.zeros(gin[fi].shape), points, V, npi)
            want[..., cc:cc + 32] += w_
            # (a point whose row is zero adds +-0: the add rounds nothing, whatever the base)
            bound[..., cc:cc + 32] = b_ + addend_count(points, V, npi, (gin[fi] != 0).any(axis=-1)) * U * np.abs(b[..., cc:cc + 32].astype(F64))
        out.append((want, bound, k))
    return out


# ---- the kernels' geometry in float32 (csrc/cnerf_dev.hpp) ----------------------------------------------------------------------------
def fma(a, b, c):
    """float32 fmaf: the product of two float32 is exact in float64."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(f32)


def linspace_at(start, end, steps, i):
    start, end, i = f32(start), f32(end), np.asarray(i)
    if steps == 1:
        return np.full(i.shape, start, f32)
    step = (end - start) / f32(steps - 1)
    return np.where(i < steps // 2, fma(step, i.astype(f32), start), fma(-step, (steps - 1 - i).astype(f32), end))


class Geom:
    def __init__(self, R, S, fov=FOV, ray_start=RAY_START, ray_end=RAY_END):
        self.R, self.S, self.NQ = R, S, (S + 3) // 4
        self.focal = f32(1.0) / f32(math.tan((2.0 * math.pi * fov / 360.0) / 2.0))
        self.ray_start, self.ray_end = f32(ray_start), f32(ray_end)
        self.half = f32(0.5) * (self.ray_end - self.ray_start) / f32(S - 1) if S > 1 else f32(0.5)

    def camera_dir(self, row, col):
        x, y = linspace_at(-1.0, 1.0, self.R, col), linspace_at(-1.0, 1.0, self.R, row)
        z = np.full(x.shape, self.focal, f32)
        n = np.sqrt(fma(z, z, fma(y, y, x * x)))
        return x / n, y / n, z / n

    def coarse_sample(self, m, d, s, u):
        """World positions (n, 3) of samples s with jitter draws u on rays of camera directions d; m: cam2world (4, 4) float32."""
        zl = linspace_at(self.ray_start, self.ray_end, self.S, s)
        dz01 = linspace_at(self.ray_start, self.ray_end, self.S, np.array(1)) - linspace_at(self.ray_start, self.ray_end, self.S, np.array(0))
        off = (np.asarray(u, f32) - f32(0.5)) * dz01
        c = [d[i] * zl + off * d[i] for i in range(3)]
        return np.stack([fma(m[r, 2], c[2], fma(m[r, 1], c[1], m[r, 0] * c[0])) + m[r, 3] for r in range(3)], -1)

    def fine_sample(self, m, d, t):
        w = [fma(m[r, 2], d[2], fma(m[r, 1], d[1], m[r, 0] * d[0])) for r in range(3)]
        return np.stack([m[r, 3] + w[r] * np.asarray(t, f32) for r in range(3)], -1)

    def positions(self, pss, m, draws, nn):
        """Positions (len(nn), 3) float32 of the points nn = ray * S + s of one image: tile_point() of the ray passes.
        draws: u_strat (pass 0) or fine_z (pass 1) of the image, (R * R * S,)."""
        nn = np.asarray(nn)
        ray, s = nn // self.S, nn % self.S
        d = self.camera_dir(ray // self.R, ray % self.R)
        return self.coarse_sample(m, d, s, draws[nn]) if pss == 0 else self.fine_sample(m, d, draws[nn])

    def depth_bin(self, t):
        """depth_bin() of scatter_patch.hip, and the distance of t to the nearest bin edge (in depth units, float64)."""
        t = np.asarray(t, f32)
        lo, width = self.ray_start - self.half, (self.ray_end - self.ray_start) + f32(2.0) * self.half
        x = (t - lo) / width * f32(self.NQ)
        q = np.clip(np.floor(x), 0.0, float(self.NQ - 1)).astype(np.int64)
        x64 = (t.astype(F64) - float(lo)) / float(width) * self.NQ
        return q, np.abs(x64 - np.rint(x64)) * float(width) / self.NQ

    def window_origin(self, pss, m, pr, pc, q, V):
        """Smallest voxel index per axis over the 8 corners of the patch-bin's frustum piece."""
        R, S = self.R, self.S
        tid = np.arange(8)
        rc = np.where(tid & 1, min(pr * 8 + 7, R - 1), pr * 8)
        cc = np.where(tid & 2, min(pc * 8 + 7, R - 1), pc * 8)
        d = self.camera_dir(rc, cc)
        far = (tid & 4) != 0
        if pss == 1:
            wbin = ((self.ray_end - self.ray_start) + f32(2.0) * self.half) / f32(self.NQ)
            p = self.fine_sample(m, d, (self.ray_start - self.half) + wbin * (q + far).astype(f32))
        else:
            p = self.coarse_sample(m, d, np.where(far, min(4 * q + 3, S - 1), 4 * q), far.astype(f32))
        return unnormalize(p, V)[0].min(axis=0)


def unnormalize(p, V):
    """i0 (n, 3) int64, lo, hi (n, 3) float32 of positions p (n, 3) float32: unnormalize() of cnerf_dev.hpp."""
    ic = ((np.asarray(p, f32) / f32(HALF_VOXEL) + f32(1.0)) * f32(V) - f32(1.0)) / f32(2.0)
    ic = np.minimum(np.maximum(ic, f32(0.0)), f32(V - 1))
    fl = np.floor(ic)
    return fl.astype(np.int64), ic - fl, (fl + f32(1.0)) - ic


# ---- the block decomposition ----------------------------------------------------------------------------------------------------------
def blocks(geom, pss, fine_z=None, unmasked_last_quad=False):
    """[(pr, pc, q, [("batch" | "direct", point indices nn)])] of one image, the waves taken in order (their order at the queue's
    counter is free on the hardware: it changes which points share a batch, never their number).  fine_z: (R * R * S,) of the image."""
    R, S, NQ = geom.R, geom.S, geom.NQ
    P = (R + 7) // 8
    bins = geom.depth_bin(fine_z)[0] if pss == 1 else None
    out = []
    for pr in range(P):
        for pc in range(P):
            r = np.arange(64)
            row, col = pr * 8 + r // 8, pc * 8 + r % 8
            ray = (row * R + col)[(row < R) & (col < R)]
            for q in range(NQ):
                work, queue = [], np.zeros(0, np.int64)

                def drain(last):
                    nonlocal queue
                    while len(queue) >= PTS or (last and len(queue)):
                        n = min(len(queue), PTS)
                        work.append(("direct" if n <= DIRECT else "batch", queue[:n]))
                        queue = queue[n:]

                for j in (range(NQ) if pss == 1 else [q]):            # rounds: one quad of samples per ray
                    s = 4 * j + np.arange(4)
                    nn = (ray[:, None] * S + s[None, :]).reshape(-1)
                    ok = np.broadcast_to(s[None, :] < S, (len(ray), 4)).reshape(-1)
                    if unmasked_last_quad:
                        ok = nn < R * R * S
                    if pss == 1:
                        ok = ok & (bins[np.minimum(nn, R * R * S - 1)] == q)
                    assert len(queue) + ok.sum() <= RING, "the ring queue would overflow"
                    queue = np.concatenate([queue, nn[ok]])
                    drain(j == NQ - 1 or pss == 0)
                out.append((pr, pc, q, work))
    return out


def populations(geom, pss, fine_z=None):
    """{(pr, pc, q): [size of every batch / direct tail]} and the partition check: every point of the image claimed exactly once."""
    claimed = np.zeros(geom.R * geom.R * geom.S, np.int64)
    pop = {}
    for pr, pc, q, work in blocks(geom, pss, fine_z):
        for kind, nn in work:
            np.add.at(claimed, nn, 1)
        pop[(pr, pc, q)] = [(kind, len(nn)) for kind, nn in work]
    assert (claimed == 1).all(), "a point is claimed by no block or by several"
    return pop


# ---- a float32 emulation of the kernel, honest or with one hazard ----------------------------------------------------------------------
HAZARDS = ("dropped_tail", "batch_twice", "clamped_twin", "image0_rows", "tile0_rows", "origin_off_by_one", "unmasked_last_quad",
           "run_across_half_waves_once")


def emulate(geom, pss, cams, draws, gin, tiles, base, hazard=None):
    """The volumes after one call, float32: cams (n_images, 4, 4), draws (n_images, npi) u_strat / fine_z, gin (feature tiles,
    n_images, npi, 32), base [(n_images, V, V, V, C)].  Records sorted by voxel, sequential run sums, one add per run and half-wave,
    direct adds for the points outside the window and the short tails."""
    assert hazard is None or hazard in HAZARDS
    vols = [b.astype(f32).copy() for b in base]
    npi = geom.R * geom.R * geom.S
    for b in range(cams.shape[0]):
        m = cams[b].astype(f32)
        blks = blocks(geom, pss, draws[b] if pss == 1 else None, hazard == "unmasked_last_quad")
        seen_batches = 0
        for fi, (lvl, cc) in enumerate(tiles):
            V = vols[lvl].shape[1]
            gv = vols[lvl][b].reshape(V ** 3, -1)[:, cc:cc + 32]
            rows_of = gin[0 if hazard == "tile0_rows" else fi][0 if hazard == "image0_rows" else b]
            for pr, pc, q, work in blks:
                o = geom.window_origin(pss, m, pr, pc, q, V)
                for kind, nn in work:
                    if kind == "direct" and hazard == "dropped_tail":
                        continue
                    i0, lo, hi = unnormalize(geom.positions(pss, m, draws[b], nn), V)
                    one = (i0 + 1 < V).astype(np.int64)
                    rel = i0 - o
                    inside = ((rel >= 0) & (rel + one < BOX)).all(axis=1) & (kind == "batch")
                    rows = rows_of[nn]
                    for rep in range(2 if kind == "batch" and hazard == "batch_twice" and seen_batches == 1 else 1):
                        recs = []                                                        # (window voxel, point of the batch, weight)
                        for k in range(8):
                            d = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1])
                            w = (np.where(d[0], lo[:, 0], hi[:, 0]) * np.where(d[1], lo[:, 1], hi[:, 1])) * np.where(d[2], lo[:, 2], hi[:, 2])
                            act = inside & ((one >= d).all(axis=1))
                            vox = ((rel[:, 2] + d[2]) * BOX + rel[:, 1] + d[1]) * BOX + rel[:, 0] + d[0]
                            recs += [(int(vox[e]), int(e), w[e]) for e in np.nonzero(act)[0]]
                            if hazard == "clamped_twin" and d[0]:                        # the clamped x + 1 corner, with corner k - 1's weight
                                w0 = (hi[:, 0] * np.where(d[1], lo[:, 1], hi[:, 1])) * np.where(d[2], lo[:, 2], hi[:, 2])
                                bad = inside & (one[:, 0] == 0) & ((one >= d * [0, 1, 1]).all(axis=1))
                                recs += [(int(vox[e]) - 1, int(e), w0[e]) for e in np.nonzero(bad)[0]]
                            # outside the window: the 8 clamped corners of trilinear_corners, one add each
                            idx = np.minimum(i0 + d, V - 1)
                            for e in np.nonzero(~inside)[0]:
                                gv[(idx[e, 2] * V + idx[e, 1]) * V + idx[e, 0]] += rows[e] * w[e]
                        recs.sort(key=lambda t: t[0])
                        total = len(recs)
                        oo = o + 1 if hazard == "origin_off_by_one" else o
                        for hw in range(8):
                            first, last = total * hw // 8, total * (hw + 1) // 8
                            cur, acc, skip = -1, None, False

                            def flush():
                                if not skip:
                                    x, y, z = (min(int(oo[a]) + ((cur >> (3 * a)) & 7), V - 1) for a in range(3))      # (min: the hazard's shift)
                                    gv[(z * V + y) * V + x] += acc

                            for i in range(first, last):
                                vox, e, w = recs[i]
                                if vox != cur:
                                    if cur >= 0:
                                        flush()
                                    # the hazard: the second half of a run that began in the previous half-wave's share is never added
                                    skip = hazard == "run_across_half_waves_once" and i == first and first > 0 and recs[first - 1][0] == vox
                                    cur, acc = vox, np.zeros(32, f32)
                                acc = acc + rows[e] * w
                            if cur >= 0:
                                flush()
                    seen_batches += kind == "batch"
    return vols


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def level_shapes(variant, V):
    """[(side, channels)] of the variant's volume levels at side V, and [(level, first channel)] of its feature input tiles."""
    lv = [(V, 32), (max(V // 2, 2), 64), (max(V // 4, 2), 32)] if variant.endswith("Pyrmd") else [(V, 32)]
    return lv, [(i, c) for i, (_, ch) in enumerate(lv) for c in range(0, ch, 32)]


def _split_depths(rng, n, n_low, low, high):
    """n depths in random order: n_low of them uniform in `low`, the others in `high`."""
    z = np.concatenate([rng.uniform(*low, n_low), rng.uniform(*high, n - n_low)])
    return z[rng.permutation(n)].astype(f32)


def fine_depths(name, B, R, S):
    """fine_z (B, R * R * S) float32 of a fine-pass case: unsorted along every ray, by design of the case."""
    rng = np.random.default_rng(len(name) * 1000 + S)
    n = R * R * S
    g = Geom(R, S)
    edges = float(g.ray_start - g.half) + (float(g.ray_end - g.ray_start) + 2 * float(g.half)) / g.NQ * np.arange(g.NQ + 1)
    inside = lambda q: (edges[q] + 0.01, edges[q + 1] - 0.01)
    if name == "fine_tail_44":            # NQ = 2.  image 1: 300 | 212, image 2: 256 | 256; image 0 is outside the chunk
        z = [rng.uniform(0.3, 1.9, n).astype(f32), _split_depths(rng, n, 300, inside(0), inside(1)), _split_depths(rng, n, 256, inside(0), inside(1))]
    elif name == "fine_ring_1536":        # NQ = 6.  image 0: everything in bin 2; image 1: 800 below ray_start (bin 0), 736 above ray_end (bin 5)
        z = [rng.uniform(*inside(2), n).astype(f32), _split_depths(rng, n, 800, (0.02, 0.2), (2.0, 2.2))]
    else:                                 # every bin populated, no depth within 0.002 of a bin edge
        q = rng.integers(0, g.NQ, (B, n))
        z = list((edges[q] + 0.002 + rng.random((B, n)) * (edges[q + 1] - edges[q] - 0.004)).astype(f32))
    z = np.stack(z)
    assert z.shape == (B, n)
    return z


#         name                  variant              B  R   S   V  pass image0 n_images
CASES = {
    "coarse_sparse_v40":   ("SHORTSIREN_FG",       2, 11, 10, 40, 0, 0, 2),
    "coarse_one_window":   ("SHORTSIREN_FG",       1, 8,  8,  6,  0, 0, 1),
    "coarse_image_range":  ("SHORTSIREN_FG",       3, 9,  5,  24, 0, 1, 2),
    "fine_tail_44":        ("SHORTSIREN_FG",       3, 8,  8,  12, 1, 1, 2),
    "fine_ring_1536":      ("SHORTSIREN_FG",       2, 8,  24, 12, 1, 0, 2),
    "fine_second_round":   ("SHORTSIREN_FG",       1, 8,  72, 12, 1, 0, 1),
    "pyramid_coarse":      ("SHORTSIREN_FG_Pyrmd", 1, 9,  6,  12, 0, 0, 1),
    "pyramid_fine":        ("SHORTSIREN_FG_Pyrmd", 1, 9,  6,  12, 1, 0, 1),
    "dgx_coarse":          ("TALLSIREN_dgx",       1, 9,  6,  12, 0, 0, 1),
    "dgx_fine":            ("TALLSIREN_dgx",       1, 9,  6,  12, 1, 0, 1),
}


def cameras(B, seed):
    """cam2world (B, 4, 4) float32 of random cameras on the CPU, as the render tests draw them."""
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix, sample_camera_positions
    torch.manual_seed(seed)
    return create_cam2world_matrix(sample_camera_positions("cpu", "y", 0.7, 1.5, B), "y").numpy().astype(f32)


def case_inputs(name, one_hot=False):
    """Everything of a case but the positions: dict(variant, B, R, S, V, pss, image0, n_images, levels, tiles, cams (B, 4, 4), u_strat
    (B, npi), fine_z (B, npi) or None, gin (feature tiles, n_images, npi, 32), base [(n_images, V, V, V, C)])."""
    variant, B, R, S, V, pss, image0, n_images = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    npi = R * R * S
    levels, tiles = level_shapes(variant, V)
    gin = rng.standard_normal((len(tiles), n_images, npi, 32)).astype(f32)
    if one_hot:                           # a single non-zero row per image (the same point in every feature tile)
        keep = rng.integers(0, npi, n_images)
        hot = np.zeros_like(gin)
        for b in range(n_images):
            hot[:, b, keep[b]] = gin[:, b, keep[b]]
        gin = hot
    base = [(0.5 * rng.standard_normal((n_images, v, v, v, c))).astype(f32) for v, c in levels]
    return dict(variant=variant, B=B, R=R, S=S, V=V, pss=pss, image0=image0, n_images=n_images, levels=levels, tiles=tiles,
                cams=cameras(B, 5 + len(name)), u_strat=rng.random((B, npi)).astype(f32), fine_z=fine_depths(name, B, R, S) if pss == 1 else None,
                gin=gin, base=base)
