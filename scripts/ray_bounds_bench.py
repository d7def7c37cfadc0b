#!/usr/bin/env python3
"""Occupancy-masked ImplicitGenerator3d.render_rays with and without per-ray sampling bounds (informational; no gate, no ratio fixed in
advance).

The scene and the masks are those of scripts/occupancy_bench.py: batch 8, 128 x 128 rays from pinhole_rays, SHORTSIREN_FG at H = 256 on a
64^3 volume, relu / no noise, SYNTHETIC ball masks (G = 64, box lo = -1, side = 2) whose radius is bisected until about 100 / 50 / 25 / 10 %
of the coarse samples of a 64-sample render are live.  Per mask and S in {16, 32, 64} (S + S samples, hierarchical):

  * the time of the masked render with the coarse samples over [ray_start, ray_end] and over the per-ray [near, far] of
    gen.ray_bounds(grid, ..., pad = --pad-cells cell edges; 0.5, ray_bounds' own default, unless given), the bounds computed once outside
    the timed call, as a camera loop would;
  * the time of the traversal (ops.occupancy_ray_bounds) alone;
  * the mean absolute pixel error of each against the unbounded S = 128 masked render of the same scene and mask (the best image the
    S <= 128 limit allows; it has sampling error of its own, which is the floor of these numbers);
  * the share of the coarse samples each gave to the field.

Philox draws with one fixed key, so every render of a row sees the same stream.  Device events around whole calls, warm-up, median of
--steps >= 10; the two calls alternate inside one loop.  Every precision runs in a child process of its own under a time limit; the first
child that fails ends the run.

    python scripts/ray_bounds_bench.py [--steps 12] [--warmup 3] [--pad-cells 0.5] [--out profiles/ray_bounds.md]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from occupancy_bench import FOV, G, LO, PRECISIONS, RAY_END, RAY_START, SIDE, TARGETS, ball_bits      # noqa: E402  (the same scene and masks)

SAMPLES = (16, 32, 64)
REFERENCE_S = 128
SIZING_S = 64
PHILOX = (0x9E3779B97F4A7C15, 3)
CHILD_TIMEOUT_S = 400


def child(args):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops
    from cnerf_amd.generators import ImplicitGenerator3d
    from cnerf_amd.generators.volumetric_rendering import pinhole_rays
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, R = args.batch, args.img_size
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, 256).to(dev)
    gen.set_device(dev)
    gen.eval()
    gen.siren.precision = args.child
    z = (torch.randn(B, 32, 64, 64, 64, device=dev), torch.randn(B, 256, device=dev))
    cam = torch.eye(4, device=dev).unsqueeze(0).repeat(B, 1, 1)
    cam[:, 2, 3] = -1.0
    origins, dirs = pinhole_rays(cam, R, FOV)
    kw = dict(clamp_mode="relu", nerf_noise=0.0, white_back=True)
    zl = torch.linspace(RAY_START, RAY_END, SIZING_S, device=dev)
    pts = (origins.unsqueeze(2) + dirs.unsqueeze(2) * zl.reshape(1, 1, SIZING_S, 1)).reshape(B, -1, 3).contiguous()

    def coarse_share(radius):
        counts = ops.occupancy_compact(ops.OccupancyGrid(ball_bits(radius, B, dev), (LO,) * 3, SIDE, G), pts)[2]
        return counts.sum().item() / (B * pts.shape[1])

    def run(grid, S, bounds):
        aux = {}
        extra = {} if bounds is None else dict(ray_near=bounds[0], ray_far=bounds[1])
        with torch.no_grad():
            px, _ = gen.render_rays(z, origins, dirs, RAY_START, RAY_END, S, True, occupancy=grid, _aux=aux, _rng={"philox": PHILOX}, **extra, **kw)
        return px, aux

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    med = lambda v: sorted(v)[len(v) // 2]
    for target in TARGETS:
        if target >= 1.0:
            radius = float(G)
        else:
            lo_r, hi_r = 0.0, float(G)
            for _ in range(20):
                radius = 0.5 * (lo_r + hi_r)
                lo_r, hi_r = (radius, hi_r) if coarse_share(radius) < target else (lo_r, radius)
        grid = ops.OccupancyGrid(ball_bits(radius, B, dev), (LO,) * 3, SIDE, G)
        bounds_of = lambda: gen.ray_bounds(grid, origins, dirs, RAY_START, RAY_END, pad=args.pad_cells * SIDE / G)
        for _ in range(args.warmup):
            bounds_of()
        torch.cuda.synchronize()
        t_bounds = [timed(bounds_of)[0] for _ in range(args.steps)]
        near, far, hit = bounds_of()
        span = ((far - near)[hit.bool()].mean().item() / (RAY_END - RAY_START)) if hit.any() else float("nan")
        reference = run(grid, REFERENCE_S, None)[0]
        for S in SAMPLES:
            paths = {"unbounded": None, "bounded": (near, far)}
            for b in paths.values():
                for _ in range(args.warmup):
                    run(grid, S, b)
            torch.cuda.synchronize()
            ms, last = {k: [] for k in paths}, {}
            for _ in range(args.steps):
                for k, b in paths.items():
                    t, last[k] = timed(lambda: run(grid, S, b))
                    ms[k].append(t)
            n = B * R * R * S
            row = dict(precision=args.child, target_share=target, ball_radius_cells=round(radius, 2), S=S, hit_share=round(hit.float().mean().item(), 4),
                       mean_span_of_hit_rays=round(span, 4), bounds_ms=round(med(t_bounds), 4), pad_cells=args.pad_cells, batch=B, img_size=R, steps=args.steps)
            for k in paths:
                px, aux = last[k]
                row[k + "_ms"] = round(med(ms[k]), 3)
                row[k + "_ms_min_max"] = [round(min(ms[k]), 3), round(max(ms[k]), 3)]
                row[k + "_live_coarse"] = round(int(aux["live_coarse"].sum()) / n, 4)
                row[k + "_live_fine"] = round(int(aux["live_fine"].sum()) / n, 4)
                row[k + "_mean_abs_err"] = float(f"{(px - reference).abs().mean().item():.4e}")
                row[k + "_max_abs_err"] = float(f"{(px - reference).abs().max().item():.4e}")
            print(json.dumps(row), flush=True)


def report(rows, args):
    out = ["# Masked ray renders with and without per-ray sampling bounds (`scripts/ray_bounds_bench.py`)", "",
           f"1x MI355X, batch {args.batch}, {args.img_size} x {args.img_size} rays from `pinhole_rays`, S + S samples, `SHORTSIREN_FG` H = 256 on a 64^3 "
           "volume, relu, no noise, Philox draws with one key.  The synthetic ball masks of `profiles/occupancy_render.md` (G = 64, box lo = -1, "
           f"side = 2), sized on the coarse samples of a {SIZING_S}-sample render.  `unbounded`: `render_rays(..., occupancy=grid)`; `bounded`: the same call "
           f"with `ray_near` / `ray_far` from `gen.ray_bounds(grid, ...)` (pad = {args.pad_cells} cell edges), computed once outside the timed call; `bounds ms`: "
           f"that traversal alone.  Error: mean |pixels - reference| over the image, the reference being the unbounded S = {REFERENCE_S} masked render of "
           "the same scene and mask (pixels in [-1, 1]; the reference has sampling error of its own, and the network is untrained: its density "
           "is noise-like inside the ball, so these errors say how fast each placement converges, not what a trained scene looks like).  "
           f"`live coarse`: share of the coarse samples given to the field.  Device events around whole calls, {args.warmup} warm-up calls, median of "
           f"{args.steps}, the two calls alternating.  Nothing here is a gate.", "",
           "| precision | target | hit rays | span | S | unbounded ms | bounded ms | bounds ms | live coarse unb. | live coarse bnd. | err unbounded | err bounded |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['precision']} | {r['target_share'] * 100:.0f} % | {r['hit_share'] * 100:.1f} % | {r['mean_span_of_hit_rays'] * 100:.0f} % | {r['S']} | "
                   f"{r['unbounded_ms']:.2f} | {r['bounded_ms']:.2f} | {r['bounds_ms']:.3f} | {r['unbounded_live_coarse'] * 100:.1f} % | "
                   f"{r['bounded_live_coarse'] * 100:.1f} % | {r['unbounded_mean_abs_err']:.3e} | {r['bounded_mean_abs_err']:.3e} |")
    out += ["", "`span`: mean length of [near, far] over the rays that hit, as a share of [ray_start, ray_end].", "", "Raw rows:", "", "```"]
    out += [json.dumps(r) for r in rows] + ["```", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pad-cells", type=float, default=0.5, help="pad of the bounds in cell edges (0.5: the default of ray_bounds)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.steps >= 10, "median of at least 10 timed calls"
    if args.child:
        return child(args)
    rows = []
    for precision in PRECISIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", precision, "--batch", str(args.batch), "--img-size", str(args.img_size),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--pad-cells", str(args.pad_cells)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S)      # a child that hangs raises here: nothing more is started
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"{precision}: child ended with status {p.returncode}; nothing more is started")
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    text = report(rows, args)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
