#!/usr/bin/env python
"""Times of the nearest-point search (cnerf_nearest_points) and of a torch baseline on the same card (informational; no gate).

Three shapes at B = 1, (n queries, m targets): (100k, 100k) two clouds of a mesh's size; (2048, 1M) few queries against many targets,
where one block per query group leaves the card idle and the targets are cut into ranges; (1M, 100k) many queries.

Per shape, in a child process of its own with a time limit of its own: after warm-up the median (min, max) over `--steps` calls, device
events around each call, of
  kernel_auto    ops.nearest_points with target_splits = 0 (the library's choice; the workspace allocation is inside the call)
  kernel_one     the same with target_splits = 1 (no ranges, no reduce; a quarter of the calls at (2048, 1M), where one lasts 84 ms)
  torch_chunked  torch.cdist(q[i0:i1], t).min(-1) over chunks of queries whose (rows, m) matrix stays under 2 GB
and the pairs per second, the VALU instructions per pair counted from the search kernel's inner loop, and the share of the card's
non-packed fp32 issue rate that count stands for.  The two results are compared (cdist is not exact: the share of equal indices and the
largest distance difference are reported, nothing is asserted).

    python scripts/nearest_bench.py [--steps 20] [--warmup 3] [--out profiles/nearest_points_rows.json]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"mesh_100k": (100_000, 100_000), "few_queries": (2048, 1_000_000), "many_queries": (1_000_000, 100_000)}
CHILD_TIMEOUT_S = 240
CHUNK_BYTES = 2 << 30
# inner loop of nearest_search_kernel per target, for the 4 queries a lane owns (two packed pairs): 6 v_pk_add_f32 (the differences),
# 6 v_pk_mul_f32, 4 v_pk_add_f32 (the sums), 4 v_cmp_lt_f32, 8 v_cndmask_b32, 1 v_add_u32 (the target's index) = 29 for 4 pairs
VALU_PER_PAIR = 29 / 4
LANES_PER_CLOCK = 256 * 4 * 16          # CUs x SIMDs x lanes: non-packed fp32 VALU operations the card issues per clock
CLOCK_HZ = 2.4e9


def median_ms(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(x, 4) for x in (sorted(ms)[len(ms) // 2], min(ms), max(ms))]


def child(name, args):
    import ctypes as C
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, _lib as L
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    n, m = SHAPES[name]
    g = torch.Generator(device=dev).manual_seed(5)
    q = torch.rand((1, n, 3), generator=g, device=dev) * 2 - 1
    t = torch.rand((1, m, 3), generator=g, device=dev) * 2 - 1
    rows = max(1, CHUNK_BYTES // (4 * m) - 1)

    def baseline():
        d, j = [], []
        for i0 in range(0, n, rows):
            v, k = torch.cdist(q[:, i0:i0 + rows], t).min(-1)
            d.append(v)
            j.append(k)
        return torch.cat(d, 1), torch.cat(j, 1)

    nb = C.c_size_t(0)
    L.check(L.lib().cnerf_nearest_points_bytes(1, n, m, 0, C.byref(nb)), "bytes")
    auto_splits = 1 if nb.value == 0 else nb.value // (8 * n)          # each half of the workspace is 256-byte aligned: rounds down right
    d2, idx = ops.nearest_points(q, t)
    d1, idx1 = ops.nearest_points(q, t, target_splits=1)
    assert torch.equal(d2, d1) and torch.equal(idx, idx1), "the result depends on target_splits"
    bd, bj = baseline()
    row = dict(part=name, n=n, m=m, auto_splits=int(auto_splits), steps=args.steps, warmup=args.warmup, chunk_rows=rows,
               baseline_same_index_share=round(float((bj == idx).float().mean()), 6),
               baseline_max_dist_diff=float((bd - d2.sqrt()).abs().max()))
    del bd, bj
    row["kernel_auto_ms"] = median_ms(lambda: ops.nearest_points(q, t), args.warmup, args.steps)
    row["kernel_one_ms"] = median_ms(lambda: ops.nearest_points(q, t, target_splits=1), args.warmup, max(5, args.steps // 4) if name == "few_queries" else args.steps)
    row["torch_chunked_ms"] = median_ms(baseline, args.warmup, args.steps)
    pairs = float(n) * m
    best = min(row["kernel_auto_ms"][0], row["kernel_one_ms"][0])
    row["pairs_per_s"] = round(pairs / (row["kernel_auto_ms"][0] * 1e-3), 0)
    row["valu_per_pair"] = VALU_PER_PAIR
    row["share_of_fp32_issue_rate"] = round(pairs * VALU_PER_PAIR / (best * 1e-3) / (LANES_PER_CLOCK * CLOCK_HZ), 4)
    row["speedup_over_torch"] = round(row["torch_chunked_ms"][0] / row["kernel_auto_ms"][0], 2)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    if args.child:
        return child(args.child, args)
    rows = []
    for name in SHAPES:          # a fresh process per shape, each under its own time limit; a failure ends the run
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup", str(args.warmup)],
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        sys.stderr.write(out.stderr[-2000:])
        if out.returncode != 0:
            raise SystemExit(f"{name}: exit code {out.returncode}")
        for line in out.stdout.splitlines():
            if line.startswith("ROW "):
                rows.append(json.loads(line[4:]))
                print(line[4:], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
