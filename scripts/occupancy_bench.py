#!/usr/bin/env python3
"""ImplicitGenerator3d.render_rays against the same call with an occupancy grid (informational; no gate, no ratio fixed in advance).

Batch 8, 128 x 128 rays from pinhole_rays, 64 + 64 samples, SHORTSIREN_FG at H = 256 on a 64^3 volume, relu / no noise, fp32 and fp16x3.
The masks are SYNTHETIC: a ball of set bits around the origin (G = 64, box lo = -1, side = 2) whose radius is bisected until about
100 / 50 / 25 / 10 % of the coarse samples are live -- the time of a masked render depends on the live share, not on what the field
computes.  Each row records the share the two passes really evaluated (the call's live counts).  The 100 % row is the all-set grid: what
it costs over the unmasked call is the compaction, the expansion and the two stream synchronisations.

Device events around whole calls, warm-up, median of --steps >= 10; the unmasked and the masked calls alternate inside one loop.  Every
precision runs in a child process of its own under a time limit; the first child that fails ends the run.

    python scripts/occupancy_bench.py [--steps 12] [--warmup 3] [--out profiles/occupancy_render.md]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FOV, RAY_START, RAY_END = 49.134342641202636, 0.25, 1.95
LO, SIDE, G = -1.0, 2.0, 64
TARGETS = (1.0, 0.5, 0.25, 0.1)
PRECISIONS = ("fp32", "fp16x3")
CHILD_TIMEOUT_S = 240


def ball_bits(radius_cells, B, dev):
    """(B, G^3 / 32) int32: the cells whose centre lies within radius_cells of the grid's centre."""
    import torch
    c = torch.arange(G, device=dev, dtype=torch.float32) + 0.5 - G / 2
    cells = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= radius_cells ** 2
    w = (cells.reshape(-1, 32).to(torch.int64) << torch.arange(32, device=dev, dtype=torch.int64)).sum(1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w.unsqueeze(0).repeat(B, 1).contiguous()


def child(args):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops
    from cnerf_amd.generators import ImplicitGenerator3d
    from cnerf_amd.generators.volumetric_rendering import pinhole_rays
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, R, S = args.batch, args.img_size, args.num_steps
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, 256).to(dev)
    gen.set_device(dev)
    gen.eval()
    gen.rng_mode = "philox"
    gen.siren.precision = args.child
    z = (torch.randn(B, 32, 64, 64, 64, device=dev), torch.randn(B, 256, device=dev))
    cam = torch.eye(4, device=dev).unsqueeze(0).repeat(B, 1, 1)
    cam[:, 2, 3] = -1.0
    origins, dirs = pinhole_rays(cam, R, FOV)
    kw = dict(clamp_mode="relu", nerf_noise=0.0, white_back=True)
    # the coarse samples at u = 0.5, to size the balls on
    zl = torch.linspace(RAY_START, RAY_END, S, device=dev)
    pts = (origins.unsqueeze(2) + dirs.unsqueeze(2) * zl.reshape(1, 1, S, 1)).reshape(B, -1, 3).contiguous()

    def coarse_share(radius):
        counts = ops.occupancy_compact(ops.OccupancyGrid(ball_bits(radius, B, dev), (LO,) * 3, SIDE, G), pts)[2]
        return counts.sum().item() / (B * pts.shape[1])

    def run(grid):
        aux = {}
        extra = {} if grid is None else dict(occupancy=grid, _aux=aux)
        with torch.no_grad():
            gen.render_rays(z, origins, dirs, RAY_START, RAY_END, S, True, **extra, **kw)
        return aux

    for target in TARGETS:
        if target >= 1.0:
            radius = float(G)
        else:
            lo_r, hi_r = 0.0, float(G)
            for _ in range(20):
                radius = 0.5 * (lo_r + hi_r)
                lo_r, hi_r = (radius, hi_r) if coarse_share(radius) < target else (lo_r, radius)
        grid = ops.OccupancyGrid(ball_bits(radius, B, dev), (LO,) * 3, SIDE, G)
        paths = {"unmasked": None, "masked": grid}
        for g in paths.values():
            for _ in range(args.warmup):
                run(g)
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        aux = {}
        for _ in range(args.steps):
            for k, g in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = run(g)
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
                aux = out if g is not None else aux
        n = B * R * R * S
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print(json.dumps(dict(precision=args.child, target_share=target, ball_radius_cells=round(radius, 2), live_coarse=round(int(aux["live_coarse"].sum()) / n, 4),
                              live_fine=round(int(aux["live_fine"].sum()) / n, 4), unmasked_ms=round(med["unmasked"], 3), masked_ms=round(med["masked"], 3),
                              unmasked_ms_min_max=[round(min(ms["unmasked"]), 3), round(max(ms["unmasked"]), 3)],
                              masked_ms_min_max=[round(min(ms["masked"]), 3), round(max(ms["masked"]), 3)], batch=B, img_size=R, num_steps=S, steps=args.steps)),
              flush=True)


def report(rows, args):
    out = ["# Occupancy-masked ray renders against `render_rays` (`scripts/occupancy_bench.py`)", "",
           f"1x MI355X, batch {args.batch}, {args.img_size} x {args.img_size} rays from `pinhole_rays`, {args.num_steps} + {args.num_steps} samples, "
           "`SHORTSIREN_FG` H = 256 on a 64^3 volume, relu, no noise, Philox draws.  Synthetic masks: a ball of set bits (G = 64, box lo = -1, "
           "side = 2) sized on the coarse samples; `live` is the share of the samples of both passes the masked call gave to the field "
           f"(its live counts).  Device events around whole calls, {args.warmup} warm-up calls, median of {args.steps}, the two calls alternating.  The unmasked "
           "call is the parent's code path, unchanged.", "",
           "| precision | target | live coarse | live fine | live (both) | unmasked ms | masked ms | masked / unmasked |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        both = (r["live_coarse"] + r["live_fine"]) / 2
        out.append(f"| {r['precision']} | {r['target_share'] * 100:.0f} % | {r['live_coarse'] * 100:.1f} % | {r['live_fine'] * 100:.1f} % | {both * 100:.1f} % | "
                   f"{r['unmasked_ms']:.2f} | {r['masked_ms']:.2f} | {r['masked_ms'] / r['unmasked_ms']:.3f} |")
    out.append("")
    for r in rows:
        if r["target_share"] >= 1.0:
            out.append(f"{r['precision']}: the all-set grid costs {r['masked_ms'] - r['unmasked_ms']:+.2f} ms over the unmasked call "
                       f"({(r['masked_ms'] / r['unmasked_ms'] - 1) * 100:+.1f} %): two compactions, two expansions, two stream synchronisations, "
                       f"{args.batch} field launches per pass instead of one.")
    out += ["", "Raw rows:", "", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=128)
    ap.add_argument("--num-steps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.steps >= 10, "median of at least 10 timed calls"
    if args.child:
        return child(args)
    rows = []
    for precision in PRECISIONS:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", precision, "--batch", str(args.batch), "--img-size", str(args.img_size),
               "--num-steps", str(args.num_steps), "--steps", str(args.steps), "--warmup", str(args.warmup)]
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
