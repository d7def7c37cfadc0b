#!/usr/bin/env python
"""Times of the back-projection (cnerf_backproject) and of the z-buffered splat (cnerf_splat_points) against plain torch statements of
the same results, on one card; writes the table as markdown (informational; no gate).

Back-projection: V = 24 views at R = 128 (depths uniform in [0.1, 2.1], so about 85 % of the pixels are valid), colours un-normalised.
Splat: one cloud of 100,000 and one of 6,250 points (the reference's down-sampled cloud) on a sphere of radius 0.45 with 0.005 of noise,
into 24 views at R = 128 from the training shell, radius 0, 1 and 2.  Per row, after warm-up, the median (min, max) over `--steps`
windows of 10 back-to-back calls (device events around each window, the sides alternating window by window), per call, of
  kernel   ops.backproject / ops.splat_points as a user calls them (bytes query, workspace and output allocations, every launch; the
           back-projection's read-back of n as well)
  torch    the statement a user would write without them: nonzero + indexing + a batched matmul; the projection in torch and one
           scatter_reduce_(..., "amin") of int64 keys per footprint offset, then the decode
and how far the two results agree.  --alt-lib PATH times the entry alone (no allocations) in this build and in a second build of the
library, e.g. one compiled with -DCNERF_SPLAT_EARLY_OUT=0: the A/B of the early-out load.

    python scripts/reproject_bench.py [--steps 20] [--warmup 3] [--out profiles/reproject.md] [--alt-lib PATH --alt-name NAME]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, R, FOV, Z_MIN, Z_MAX = 24, 128, 49.134342641202636, 0.25, 1.95
CLOUDS = (100_000, 6_250)
RADII = (0, 1, 2)
INNER = 10       # calls inside one pair of events


def median_ms(fns, warmup, steps):
    """Per function of `fns` the [median, min, max] ms per call over `steps` windows of INNER back-to-back calls; the functions alternate
    window by window, so that a drift of the clock or a neighbour on the host meets all of them alike."""
    import torch
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / INNER)
    return [[round(x, 4) for x in (sorted(m)[len(m) // 2], min(m), max(m))] for m in ms]


def torch_backproject(pixels, depth, cams, focal):
    """inference.py:543-562 for all views at once, on the device."""
    import torch
    ok = (depth > Z_MIN) & (depth < Z_MAX)
    idx = ok.nonzero()                                                # (n,3) = v, row, col in ascending order
    z = depth[ok]
    yx = (2 * idx[:, 1:].float() - (R - 1)) / (R - 1) / focal * z[:, None]
    pts = torch.stack([yx[:, 1], yx[:, 0], z, torch.ones_like(z)], 1)
    world = torch.bmm(cams[idx[:, 0]], pts[:, :, None])[:, :3, 0]
    return torch.cat([world, pixels.permute(0, 2, 3, 1)[ok] * 0.5 + 0.5], 1)


def torch_splat(points, cams, focal, radius):
    """The same picture in plain torch: int64 keys (z > 0, so the signed order is the unsigned one), one scatter_reduce_ per offset."""
    import torch
    B, n, _ = points.shape
    Vv = cams.shape[1]
    dev = points.device
    q = points[:, None, :, :3] - cams[:, :, None, :3, 3]
    cam = torch.einsum("bvnk,bvkj->bvnj", q, cams[..., :3, :3])
    z = cam[..., 2]
    half = 0.5 * (R - 1)
    u, v = cam[..., 0] * focal / z * half + half, cam[..., 1] * focal / z * half + half
    keep = (z > Z_MIN) & (z < Z_MAX) & (u > -(radius + 1)) & (u < R + radius) & (v > -(radius + 1)) & (v < R + radius)
    col = torch.where(keep, u, torch.zeros_like(u)).round().long()
    row = torch.where(keep, v, torch.zeros_like(v)).round().long()
    key = (z.contiguous().view(torch.int32).long() << 32) | torch.arange(n, device=dev)
    empty = torch.iinfo(torch.int64).max
    keys = torch.full((B * Vv * R * R,), empty, dtype=torch.int64, device=dev)
    base = torch.arange(B * Vv, device=dev).view(B, Vv, 1) * (R * R)
    for dr in range(-radius, radius + 1):
        for dc in range(-radius, radius + 1):
            rr, cc = row + dr, col + dc
            ok = keep & (rr >= 0) & (rr < R) & (cc >= 0) & (cc < R)
            keys.scatter_reduce_(0, (base + rr * R + cc)[ok], key[ok], "amin")
    keys = keys.view(B, Vv, R, R)
    hit = keys != empty
    depth = torch.where(hit, (keys >> 32).int().view(torch.float32), torch.zeros((), device=dev))
    index = torch.where(hit, keys & 0xFFFFFFFF, torch.full((), -1, dtype=torch.int64, device=dev)).int()
    rgb = torch.gather(points[..., 3:6], 1, index.clamp(min=0).long().view(B, -1, 1).expand(-1, -1, 3)).view(B, Vv, R, R, 3)
    return depth, index, torch.where(hit[..., None], rgb, torch.ones((), device=dev))


def raw_splat(handle, points, cams, focal, radius):
    """cnerf_splat_points of the library `handle` on buffers made once: the entry alone."""
    import torch
    from cnerf_amd import _lib as L, ops
    fn = handle.cnerf_splat_points
    fn.restype, fn.argtypes = L.PROTOTYPES["cnerf_splat_points"]
    B, n, stride = points.shape
    Vv, dev = cams.shape[1], points.device
    ws = torch.empty(8 * B * Vv * R * R + 256, dtype=torch.uint8, device=dev)
    depth = torch.empty((B, Vv, R, R), dtype=torch.float32, device=dev)
    index = torch.empty((B, Vv, R, R), dtype=torch.int32, device=dev)
    pixels = torch.empty((B, Vv, R, R, 3), dtype=torch.float32, device=dev)
    c16 = cams.reshape(B, Vv, 16).contiguous()
    bg = (C.c_float * 3)(1.0, 1.0, 1.0)

    def call():
        rc = fn(B, n, stride, L.ptr(points), None, Vv, L.ptr(c16), R, focal, Z_MIN, Z_MAX, radius, bg, L.ptr(depth), L.ptr(index), L.ptr(pixels), L.ptr(ws),
                ops._stream())
        assert rc == 0, rc
    return call, (depth, index, pixels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reproject.md"))
    ap.add_argument("--alt-lib", default=None, help="a second build of libcnerf_hip.so to time the splat entry of, beside this one")
    ap.add_argument("--alt-name", default="alternative build")
    ap.add_argument("--note", default=None, help="a paragraph appended under the A/B table")
    args = ap.parse_args()
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, views, _lib as L
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    focal = views.focal_of(FOV)
    g = torch.Generator(device=dev).manual_seed(7)
    import numpy as np
    np.random.seed(7)
    cams = create_cam2world_matrix(sample_camera_positions(dev, "y", 0.7, 1.5, V), "y", dev)
    rows = []

    depth = torch.rand((V, R, R), generator=g, device=dev) * 2.0 + 0.1
    pixels = torch.rand((V, 3, R, R), generator=g, device=dev) * 2 - 1
    ours = lambda: views.fuse_depth_maps(pixels, depth, cams, FOV, Z_MIN, Z_MAX)
    base = lambda: torch_backproject(pixels, depth, cams, focal)
    a, b = ours(), base()
    row = dict(part="backproject", V=V, R=R, steps=args.steps, warmup=args.warmup, n=int(a.shape[0]), same_n=a.shape == b.shape,
               two_runs_same_bits=bool(torch.equal(a, ours())), max_abs_diff=float((a - b).abs().max()) if a.shape == b.shape else None)
    row["kernel_ms"], row["torch_ms"] = median_ms((ours, base), args.warmup, args.steps)
    row["pixels_per_s"] = round(V * R * R / (row["kernel_ms"][0] * 1e-3))
    row["kernel_over_torch"] = round(row["torch_ms"][0] / row["kernel_ms"][0], 2)
    rows.append(row)
    print(json.dumps(row), flush=True)

    alt = C.CDLL(args.alt_lib) if args.alt_lib else None
    ab = []
    for n in CLOUDS:
        d = torch.randn((1, n, 3), generator=g, device=dev)
        pcl = torch.cat([d / d.norm(dim=-1, keepdim=True) * 0.45 + torch.randn((1, n, 3), generator=g, device=dev) * 0.005,
                         torch.rand((1, n, 3), generator=g, device=dev)], -1).contiguous()
        for radius in RADII:
            ours = lambda: ops.splat_points(pcl, cams[None], R, focal, Z_MIN, Z_MAX, radius=radius)
            base = lambda: torch_splat(pcl, cams[None], focal, radius)
            a, a2, b = ours(), ours(), base()
            hit = a[1] >= 0
            row = dict(part="splat", n=n, V=V, R=R, radius=radius, steps=args.steps, warmup=args.warmup, covered_share=round(float(hit.float().mean()), 4),
                       points_per_covered_pixel=round(float(n * V * (2 * radius + 1) ** 2 / max(1, int(hit.sum()))), 2),
                       two_runs_same_bits=all(bool(torch.equal(x, y)) for x, y in zip(a, a2)),
                       index_equal_share=round(float((a[1] == b[1]).float().mean()), 8), max_depth_diff=float((a[0] - b[0]).abs().max()))
            row["kernel_ms"], row["torch_ms"] = median_ms((ours, base), args.warmup, args.steps)
            row["point_views_per_s"] = round(n * V / (row["kernel_ms"][0] * 1e-3))
            row["kernel_over_torch"] = round(row["torch_ms"][0] / row["kernel_ms"][0], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if alt is not None:
                f0, o0 = raw_splat(L.lib(), pcl, cams[None], focal, radius)
                f1, o1 = raw_splat(alt, pcl, cams[None], focal, radius)
                f0(), f1()
                r = dict(part="splat_entry_ab", n=n, radius=radius, same_bits=all(bool(torch.equal(x, y)) for x, y in zip(o0, o1)))
                r["this_build_ms"], r["alt_build_ms"] = median_ms((f0, f1), args.warmup, args.steps)
                ab.append(r)
                print(json.dumps(r), flush=True)

    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    bp = rows[0]
    md = ["# Depth maps <-> clouds: `cnerf_backproject`, `cnerf_splat_points` (`scripts/reproject_bench.py`)", "",
          f"1x MI355X (gfx950; the runtime names the device \"{torch.cuda.get_device_name(0)}\").  Device events around windows of {INNER} back-to-back calls,",
          f"{args.warmup} warm-up calls, median of {args.steps} windows per call (min .. max); the two sides of a row alternate window by window in one process.",
          "Informational: nothing here is gated.  The feature does not exist before this change, so the yardstick is the torch statement of the",
          "same result on the same card.  `DESIGN.md` 3.22 reads the figures.", "",
          f"## Back-projection: {V} views at R = {R}, {bp['n']:,} of {V * R * R:,} pixels valid", "",
          "`kernel` is `views.fuse_depth_maps` (`ops.backproject`: bytes query, allocations, three launches, the read-back of n).  `torch` is",
          "`nonzero` + boolean indexing + a batched matmul + the colours' gather.", "",
          "| kernel ms | torch ms | kernel over torch | pixels / s | two runs same bits | same n | max abs difference |", "|---|---|---|---|---|---|---|",
          f"| {f3(bp['kernel_ms'])} | {f3(bp['torch_ms'])} | {bp['kernel_over_torch']}x | {bp['pixels_per_s']:.3g} | {bp['two_runs_same_bits']} | {bp['same_n']} | {bp['max_abs_diff']} |", "",
          f"## Splat: one cloud into {V} views at R = {R}", "",
          "`kernel` is `ops.splat_points` (bytes query, allocations, the clear, both launches).  `torch` is the projection as an einsum and one",
          "`scatter_reduce_(..., \"amin\")` of int64 keys per footprint offset, then the decode.  The cloud is a sphere of radius 0.45 with 0.005 of noise.", "",
          "| points | radius | covered pixels | point footprints per covered pixel | kernel ms | torch ms | kernel over torch | point-views / s | two runs same bits | index equal share |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows[1:]:
        md.append(f"| {r['n']:,} | {r['radius']} | {r['covered_share']:.1%} | {r['points_per_covered_pixel']} | {f3(r['kernel_ms'])} | {f3(r['torch_ms'])} | "
                  f"{r['kernel_over_torch']}x | {r['point_views_per_s']:.3g} | {r['two_runs_same_bits']} | {r['index_equal_share']} |")
    slower = [f"{r['part']} n = {r.get('n')} radius {r.get('radius')} ({r['kernel_over_torch']}x)" for r in rows if r["kernel_over_torch"] < 1]
    md += ["", f"The kernel took no longer than the torch statement in {len(rows) - len(slower)} of {len(rows)} rows"
           + ("." if not slower else "; it was slower at: " + ", ".join(slower) + "."),
           "The torch statement forms u and v in its own order of operations, so a few pixels may differ (index equal share; nothing is asserted)."]
    if ab:
        md += ["", f"## The entry alone, this build against: {args.alt_name}", "",
               "`cnerf_splat_points` through ctypes on buffers made once (no allocation in the timed call), both libraries loaded in one process.", "",
               "| points | radius | this build ms | alternative ms | this build over alternative | same bits |", "|---|---|---|---|---|---|"]
        for r in ab:
            md.append(f"| {r['n']:,} | {r['radius']} | {f3(r['this_build_ms'])} | {f3(r['alt_build_ms'])} | {r['alt_build_ms'][0] / r['this_build_ms'][0]:.2f}x | {r['same_bits']} |")
    if args.note:
        md += ["", args.note]
    md += ["", "## Raw rows", "", "```"] + [json.dumps(r) for r in rows + ab] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(md))


if __name__ == "__main__":
    main()
