#!/usr/bin/env python
"""Times of the TSDF fusion (cnerf_tsdf_integrate through ops.tsdf_integrate) against the plain torch statement of the same volume, and
of what surrounds it in extract_shapes.extract_mesh_tsdf; writes the tables as markdown (informational; no gate).

Fusion: the analytic depth maps of a ball of radius 0.35 seen from a ring of look-at cameras at radius 1.4 - 1.6, fused into a cube of
side 0.9 -- lattices of 128^3 and 256^3 points, 24 views of 128^2 and 8 views of 256^2, trunc three pitches.  Per row, after `--warmup`
calls, the median (min, max) over `--steps` calls, device events around each call, the sides alternating call by call, of
  kernel   ops.tsdf_integrate as a user calls it (allocations of the outputs and the launch), without and with colours
  torch    the statement a user would write without it: a loop over the views with whole-lattice tensors (a matmul, the projection,
           a gather of the depth, masks and where), without and with colours
and how far the two volumes agree.  Every shape runs in a process of its own under its own time limit; the parent opens no GPU.

Surroundings: the 24 renders of the untrained benchmark generator (SHORTSIREN_FG, hidden 256, 128^2 pixels, 64 + 64 samples, 8 views per
batch), the fusion into 256^3, and ops.isosurface of the result -- how large the fusion's share of extract_mesh_tsdf is.

    python scripts/tsdf_bench.py [--steps 20] [--warmup 3] [--out profiles/tsdf.md] [--notes FILE]"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOV, RAY_START, RAY_END = 49.134342641202636, 0.5, 2.5
SIDE, BALL_R = 0.9, 0.35
SHAPES = ((128, 24, 128), (256, 24, 128), (128, 8, 256), (256, 8, 256))          # lattice edge, views, image edge
LIMIT_S = 240                                                                    # per child process


def ring_cameras(V, dev):
    """V look-at cameras around the origin: azimuths evenly spaced, elevations alternating +-20 degrees, radii from 1.4 to 1.6."""
    import torch
    from cnerf_amd.generators.volumetric_rendering import create_cam2world_matrix
    k = torch.arange(V, dtype=torch.float32)
    az, el = 2 * math.pi * k / V, math.radians(20.0) * (1 - 2 * (k % 2))
    r = 1.4 + 0.2 * k / max(V - 1, 1)
    o = torch.stack([r * torch.cos(el) * torch.sin(az), r * torch.sin(el), r * torch.cos(el) * torch.cos(az)], 1)
    return create_cam2world_matrix(o, "y").to(dev)


def ball_views(cams, R, focal):
    """pixels (V,3,R,R) in [-1,1] (the ball's normal, 0 off the ball) and z-depth (V,R,R), 0 where the pixel's ray misses the ball."""
    import torch
    dev = cams.device
    g = (2 * torch.arange(R, device=dev, dtype=torch.float64) - (R - 1)) / (R - 1) / focal
    d = torch.stack([g[None, :].expand(R, R), g[:, None].expand(R, R), torch.ones((R, R), device=dev, dtype=torch.float64)], -1)
    M = cams.double()
    dw = torch.einsum("rck,vjk->vrcj", d, M[:, :3, :3])
    o = M[:, None, None, :3, 3]
    a, b, c = (dw * dw).sum(-1), (dw * o).sum(-1), (o * o).sum(-1) - BALL_R ** 2
    disc = b * b - a * c
    lam = (-b - disc.clamp(min=0).sqrt()) / a
    hit = (disc > 0) & (lam > 0)
    depth = torch.where(hit, lam, torch.zeros_like(lam))
    p = dw * depth[..., None] + o
    pixels = torch.where(hit[..., None], p / BALL_R, torch.zeros_like(p)).permute(0, 3, 1, 2)
    return pixels.float().contiguous(), depth.float().contiguous()


def torch_tsdf(depth, pixels, cams, focal, N, lo, pitch, trunc):
    """The contract of cnerf_tsdf_integrate (carve, hidden_min = 1, unseen = -1) as a user would write it in torch: one view at a time
    over the whole lattice.  torch forms the sums in its own order, so the result is close to the kernel's, not its bits."""
    import torch
    dev = depth.device
    V, R, _ = depth.shape
    ax = torch.arange(N, device=dev, dtype=torch.float32) * pitch
    p = torch.stack(torch.meshgrid(ax + lo[0], ax + lo[1], ax + lo[2], indexing="ij"), -1).reshape(-1, 3)
    n = p.shape[0]
    total, cnt, hid = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    csum = torch.zeros((n, 3), device=dev) if pixels is not None else None
    cn = torch.zeros(n, device=dev) if pixels is not None else None
    half = 0.5 * (R - 1)
    for w in range(V):
        cam = (p - cams[w, :3, 3]) @ cams[w, :3, :3]
        z = cam[:, 2]
        u, v = cam[:, 0] * focal / z * half + half, cam[:, 1] * focal / z * half + half
        ok = (z > 0) & (u > -1) & (u < R) & (v > -1) & (v < R)
        col = torch.where(ok, u, torch.zeros_like(u)).round().long()
        row = torch.where(ok, v, torch.zeros_like(v)).round().long()
        ok &= (col >= 0) & (col < R) & (row >= 0) & (row < R)
        col, row = col.clamp(0, R - 1), row.clamp(0, R - 1)
        d = depth[w][row, col]
        surface = ok & (d > RAY_START) & (d < RAY_END)
        s = (z - d) / trunc
        hidden = surface & (s > 1)
        obs = surface & ~hidden
        background = ok & ~surface & ~torch.isnan(d)
        total += torch.where(obs, s.clamp(min=-1), torch.zeros_like(s)) - background.float()
        cnt += (obs | background).float()
        hid += hidden.float()
        if pixels is not None:
            band = obs & (s >= -1)
            csum += torch.where(band[:, None], pixels[w][:, row, col].T * 0.5 + 0.5, torch.zeros((), device=dev))
            cn += band.float()
    tsdf = torch.where(cnt > 0, total / cnt.clamp(min=1), torch.where(hid >= 1, torch.ones_like(total), -torch.ones_like(total))).reshape(N, N, N)
    rgb = None if pixels is None else (csum / cn.clamp(min=1)[:, None]).reshape(N, N, N, 3)
    return tsdf, rgb


def median_ms(fns, warmup, steps):
    """Per function the [median, min, max] ms over `steps` calls, device events around each call; the functions alternate."""
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
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return [[round(x, 4) for x in (sorted(m)[len(m) // 2], min(m), max(m))] for m in ms]


def fusion_row(N, V, R, warmup, steps):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, views
    dev = torch.device("cuda:0")
    focal = views.focal_of(FOV)
    cams = ring_cameras(V, dev)
    pixels, depth = ball_views(cams, R, focal)
    lo, pitch = (-SIDE / 2,) * 3, SIDE / (N - 1)
    trunc = 3 * pitch
    kw = dict(shape=(N, N, N), lo=lo, pitch=pitch, trunc=trunc)
    plain = lambda: ops.tsdf_integrate(depth, cams, focal, RAY_START, RAY_END, **kw)
    coloured = lambda: ops.tsdf_integrate(depth, cams, focal, RAY_START, RAY_END, colors=pixels, color_scale=0.5, color_offset=0.5, **kw)
    t_plain = lambda: torch_tsdf(depth, None, cams, focal, N, lo, pitch, trunc)
    t_coloured = lambda: torch_tsdf(depth, pixels, cams, focal, N, lo, pitch, trunc)
    a, a2, b = coloured(), coloured(), t_coloured()
    sign = ((a[0] > 0) == (b[0] > 0)).float().mean()
    row = dict(part="fusion", N=N, V=V, R=R, steps=steps, warmup=warmup, pairs=N ** 3 * V, two_runs_same_bits=bool(torch.equal(a[0], a2[0]) and torch.equal(a[2], a2[2])),
               plain_equals_coloured_tsdf=bool(torch.equal(plain()[0], a[0])), max_tsdf_diff_vs_torch=float((a[0] - b[0]).abs().max()),
               same_sign_share_vs_torch=round(float(sign), 8), inside_share=round(float((a[0] > 0).float().mean()), 4))
    del a, a2, b
    row["kernel_ms"], row["kernel_rgb_ms"], row["torch_ms"], row["torch_rgb_ms"] = median_ms((plain, coloured, t_plain, t_coloured), warmup, steps)
    row["pairs_per_s"] = round(row["pairs"] / (row["kernel_ms"][0] * 1e-3))
    row["pairs_per_s_rgb"] = round(row["pairs"] / (row["kernel_rgb_ms"][0] * 1e-3))
    row["torch_over_kernel"] = round(row["torch_ms"][0] / row["kernel_ms"][0], 1)
    row["torch_over_kernel_rgb"] = round(row["torch_rgb_ms"][0] / row["kernel_rgb_ms"][0], 1)
    return row


def surround_row(warmup, steps):
    """extract_mesh_tsdf's three parts on the untrained benchmark generator: 24 renders, the fusion into 256^3, the isosurface."""
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, views
    from cnerf_amd.generators import ImplicitGenerator3d
    dev = torch.device("cuda:0")
    N, V, R, S = 256, 24, 128, 64
    torch.manual_seed(0)
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, 256).to(dev)
    gen.set_device(dev)
    z = (torch.randn(1, 32, 64, 64, 64, device=dev), torch.randn(1, 256, device=dev))
    cams = ring_cameras(V, dev)
    cams[:, :3, 3] *= 0.75                                                       # radius 1.05 - 1.2: inside the training shell of 0.7 - 1.5
    meta = dict(clamp_mode="relu", nerf_noise=0.0, white_back=True, hierarchical_sample=True)
    ray_start, ray_end = 0.25, 1.95
    out = {}

    def render():
        out["views"] = views.render_views(gen, z, cams, R, FOV, ray_start, ray_end, S, views_per_batch=8, **meta)

    def fuse():
        out["vol"] = views.tsdf_volume(*out["views"], cams, FOV, ray_start, ray_end, resolution=N, cube_length=1.2)

    def mesh():
        t, _, rgb, lo, pitch = out["vol"]
        out["mesh"] = ops.isosurface(t, 0.0, lo=lo, pitch=pitch, attrs=rgb)

    steps = max(3, steps // 4)                                                   # a render pass is hundreds of ms
    ms = median_ms((render, fuse, mesh), 1, steps)
    row = dict(part="surround", N=N, V=V, R=R, num_steps=S, steps=steps, warmup=1, render_ms=ms[0], fusion_ms=ms[1], isosurface_ms=ms[2],
               vertices=int(out["mesh"][0].shape[0]), triangles=int(out["mesh"][1].shape[0]),
               surface_pixel_share=round(float(((out["views"][1] > ray_start) & (out["views"][1] < ray_end)).float().mean()), 4))
    row["fusion_share"] = round(ms[1][0] / (ms[0][0] + ms[1][0] + ms[2][0]), 5)
    return row


def child(args):
    row = surround_row(args.warmup, args.steps) if args.one == "surround" else fusion_row(*(int(x) for x in args.one.split(",")), args.warmup, args.steps)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf.md"))
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "tsdf_kernel.md"),
                    help="a markdown file appended under the tables: the kernel's resource table and instruction counts, read from the compiler")
    ap.add_argument("--one", default=None, help="run one shape 'N,V,R' (or 'surround') in this process and print its row")
    args = ap.parse_args()
    if args.one:
        return child(args)
    rows = []
    for one in [f"{N},{V},{R}" for N, V, R in SHAPES] + ["surround"]:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", one, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            sys.exit(f"{one}: no result within {LIMIT_S} s; stopping here")
        got = [ln[4:] for ln in res.stdout.splitlines() if ln.startswith("ROW ")]
        if res.returncode != 0 or not got:
            sys.exit(f"{one}: exit status {res.returncode}; stopping here\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
        rows.append(json.loads(got[0]))
        print(got[0], flush=True)

    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    md = ["# Depth maps -> a TSDF lattice: `cnerf_tsdf_integrate` (`scripts/tsdf_bench.py`)", "",
          f"1x MI355X (gfx950).  Device events around each call, {args.warmup} warm-up calls, median of {args.steps} calls (min .. max); the sides of a row",
          "alternate call by call in one process, and every row runs in a process of its own.  Informational: nothing here is gated.  The feature",
          "does not exist before this change, so the yardstick is the torch statement of the same volume on the same card.  `DESIGN.md` 3.23 reads",
          "the figures.", "",
          "## Fusion: the analytic ball (radius 0.35) into a cube of side 0.9, trunc three pitches", "",
          "`kernel` is `ops.tsdf_integrate` (output allocations and one launch), `torch` a loop over the views with whole-lattice tensors.",
          "A pair is one voxel projected into one view.", "",
          "| lattice | views | kernel ms | kernel + colours ms | torch ms | torch + colours ms | torch over kernel | with colours | pairs / s | with colours | two runs same bits | max tsdf difference to torch | same sign share |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["part"] == "fusion":
            md.append(f"| {r['N']}^3 | {r['V']} x {r['R']}^2 | {f3(r['kernel_ms'])} | {f3(r['kernel_rgb_ms'])} | {f3(r['torch_ms'])} | {f3(r['torch_rgb_ms'])} | "
                      f"{r['torch_over_kernel']}x | {r['torch_over_kernel_rgb']}x | {r['pairs_per_s']:.3g} | {r['pairs_per_s_rgb']:.3g} | {r['two_runs_same_bits']} | "
                      f"{r['max_tsdf_diff_vs_torch']:.3g} | {r['same_sign_share_vs_torch']} |")
    md += ["", "torch forms the projection with a matmul and its sums in its own order: a few voxels read a neighbouring pixel (nothing is asserted)."]
    for r in rows:
        if r["part"] == "surround":
            md += ["", "## What surrounds the fusion in `extract_mesh_tsdf`", "",
                   f"The untrained benchmark generator (SHORTSIREN_FG, hidden 256, a 64^3 feature volume): {r['V']} views of {r['R']}^2 pixels, {r['num_steps']} + {r['num_steps']}",
                   f"samples per ray, 8 views per batch; the fusion into {r['N']}^3 with colours; `ops.isosurface` of the result ({r['vertices']:,} vertices, {r['triangles']:,}",
                   f"triangles; {r['surface_pixel_share']:.1%} of the pixels are surface).  Median of {r['steps']} after one warm-up.", "",
                   "| 24 renders ms | fusion ms | isosurface ms | the fusion's share |", "|---|---|---|---|",
                   f"| {f3(r['render_ms'])} | {f3(r['fusion_ms'])} | {f3(r['isosurface_ms'])} | {r['fusion_share']:.2%} |"]
    if args.notes and os.path.exists(args.notes):
        md += ["", open(args.notes).read().rstrip()]
    md += ["", "## Raw rows", "", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(md))


if __name__ == "__main__":
    main()
