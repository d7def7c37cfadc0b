#!/usr/bin/env python
"""Times of the two stable compactions alone (informational; no gate): ops.occupancy_compact (count, scan, rank) and ops.backproject
(count, scan, emit), which the other scripts time only inside a render or beside a torch statement.

Compaction: B = 8 images of 128 x 128 x 64 = 1,048,576 points uniform over 1.2 x the box [-1, 1]^3, a ball mask of radius 25 cells at
G = 64, rank and live_points allocated beforehand.  Back-projection: 24 views of 128 x 128 with colours, depths uniform in [0.1, 2.1].
Per row, after 3 warm-up calls, the median (min, max) ms per call over `--steps` windows of 10 back-to-back calls, device events around
each window.  To compare two builds, run the script once in each checkout, alternating.

    python scripts/compaction_bench.py [--steps 30]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INNER = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    G, B, n = 64, 8, 128 * 128 * 64
    c = torch.arange(G, device=dev, dtype=torch.float32) + 0.5 - G / 2
    cells = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) <= 25.0 ** 2
    w = (cells.reshape(-1, 32).to(torch.int64) << torch.arange(32, device=dev, dtype=torch.int64)).sum(1)
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).unsqueeze(0).repeat(B, 1).contiguous()
    grid = ops.OccupancyGrid(w, (-1.0,) * 3, 2.0, G)
    pts = (torch.rand((B, n, 3), device=dev) * 2.4 - 1.2).contiguous()
    rank = torch.empty((B, n), dtype=torch.int32, device=dev)
    live = torch.empty((B, n, 3), dtype=torch.float32, device=dev)
    V, R = 24, 128
    depth = torch.rand((V, R, R), device=dev) * 2.0 + 0.1
    colors = torch.rand((V, 3, R, R), device=dev)
    cams = torch.eye(4, device=dev).unsqueeze(0).repeat(V, 1, 1).contiguous()
    parts = (("occupancy_compact", lambda: ops.occupancy_compact(grid, pts, rank=rank, live_points=live)),
             ("backproject", lambda: ops.backproject(depth, cams, 2.1875, 0.25, 1.95, colors=colors)))
    for name, fn in parts:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(INNER):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / INNER)
        ms.sort()
        print(json.dumps(dict(part=name, steps=args.steps, ms=[round(x, 4) for x in (ms[len(ms) // 2], ms[0], ms[-1])])), flush=True)


if __name__ == "__main__":
    main()
