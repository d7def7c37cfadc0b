#!/usr/bin/env python
"""Times of connected-component labelling of a lattice on the device (cnerf_components_label / _filter through ops.connected_components and
ops.keep_components) against what a user would write without them; writes the table as markdown (informational; no gate).

Lattices, each at 128^3 and 256^3 points (the path: 127 x 127 x 128 and 255 x 255 x 256), selection v > 0:
  ball    a ball of radius 0.3 in the unit cube and 300 small balls (radius 0.02) around it: one large solid and floaters
  noise   white noise smoothed twice over 3 x 3 x 3, thresholded at one deviation: thousands of components of every size
  path    one path that winds through the whole lattice, rows two apart joined end to end: a single chain of N^3 / 4 + N^2 / 4 - 1 points
Per row, after `--warmup` calls, the median (min, max) over `--steps` calls, device events around each call, of
  label           ops.connected_components as a user calls it (allocations of the three outputs and the workspace, five launches)
  label + filter  ops.keep_components (that, the output lattice and one more launch)
and once each (they take long), with the same neighbour offsets,
  torch           minimum-label propagation in torch until nothing changes: per sweep 14 shifted minima over the whole lattice, the
                  convergence test (one readback) every 8 sweeps; at most `--max-sweeps` sweeps, and the row says if that was not enough
  scipy           scipy.ndimage.label with the same structure, including the copy to the host and the labels' copy back (if scipy imports)
Every row runs in a process of its own under its own time limit; the parent opens no GPU.  Before the timed calls a row makes one call
alone and stops if that took more than `--give-up-ms`: a lattice that the union-find handles badly is reported, not waited for.

    python scripts/components_bench.py [--steps 20] [--warmup 3] [--out profiles/components.md] [--notes FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = [(1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
ROWS = [f"{kind},{N}" for N in (128, 256) for kind in ("ball", "noise", "path")]
LIMIT_S = 420                                                                    # per child process


def lattice(kind, N, dev):
    import torch
    g = torch.Generator(device="cpu").manual_seed(N)
    if kind == "ball":
        ax = torch.arange(N, device=dev, dtype=torch.float32) / (N - 1)
        x = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
        v = 0.3 ** 2 - ((x - 0.5) ** 2).sum(-1)
        for c in torch.rand((300, 3), generator=g).mul(0.9).add(0.05).tolist():
            if sum((t - 0.5) ** 2 for t in c) ** 0.5 < 0.36:
                continue
            lo = [max(0, int((t - 0.03) * (N - 1))) for t in c]
            hi = [min(N, int((t + 0.03) * (N - 1)) + 2) for t in c]
            box = (slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2]))
            v[box] = torch.maximum(v[box], 0.02 ** 2 - ((x[box] - torch.tensor(c, device=dev)) ** 2).sum(-1))
        return v.contiguous()
    if kind == "noise":
        v = torch.randn((N, N, N), generator=g).to(dev)
        for _ in range(2):
            for ax in range(3):
                v = (torch.roll(v, 1, ax) + v + torch.roll(v, -1, ax)) / 3.0
        return (v / v.std() - 1.0).contiguous()
    A = N // 2                                                                   # path: tests/components_common.py's winding_path, on the device
    v = torch.full((2 * A - 1, 2 * A - 1, N), -1.0, device=dev)
    v[::2, ::2, :] = 1.0
    a = torch.arange(A, device=dev)
    k = torch.arange(A - 1, device=dev)
    # row k of a plane (in the order it is walked) ends at i2 = N - 1 for even k + a A, else at 0; the joint after it sits there
    for par in (0, 1):
        aa = a[par::2]
        kk, ka = torch.meshgrid(k, aa, indexing="ij")
        b = kk if par == 0 else A - 1 - kk
        end = torch.where((kk + ka * A) % 2 == 0, N - 1, 0)
        v[2 * ka, 2 * b + (1 if par == 0 else -1), end] = 1.0
    last_b = torch.where(a[:-1] % 2 == 0, A - 1, 0)
    end = torch.where((A - 1 + a[:-1] * A) % 2 == 0, N - 1, 0)
    v[2 * a[:-1] + 1, 2 * last_b, end] = 1.0
    assert int((v > 0).sum()) == A * A * N + A * A - 1             # winding_path's count: A^2 rows of N points and A^2 - 1 joints
    return v.contiguous()


def torch_labels(v, max_sweeps):
    """Minimum-label propagation over the 14 neighbours until nothing changes -> labels (-1 off the selection), sweeps, converged."""
    import torch
    sel = v > 0
    n = v.numel()
    lab = torch.where(sel, torch.arange(n, device=v.device, dtype=torch.int32).reshape(v.shape), torch.full((), n, dtype=torch.int32, device=v.device))
    sweeps, done = 0, False
    while sweeps < max_sweeps and not done:
        before = lab.clone()
        for _ in range(8):
            for d in KINDS:
                own = tuple(slice(0, s - dd) for s, dd in zip(v.shape, d))
                oth = tuple(slice(dd, s) for s, dd in zip(v.shape, d))
                m = torch.minimum(lab[own], lab[oth])
                both = sel[own] & sel[oth]
                lab[own] = torch.where(both, m, lab[own])
                lab[oth] = torch.where(both, torch.minimum(m, lab[oth]), lab[oth])
            sweeps += 1
        done = bool(torch.equal(before, lab))
    return torch.where(sel, lab, torch.full((), -1, dtype=torch.int32, device=v.device)), sweeps, done


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


def row_of(kind, N, args):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops
    dev = torch.device("cuda:0")
    v = lattice(kind, N, dev)
    label = lambda: ops.connected_components(v, 0.0)
    keep = lambda: ops.keep_components(v, 0.0)
    first = median_ms(label, 0, 1)
    labels, sizes, stats = label()
    st = stats.tolist()
    row = dict(kind=kind, N=N, shape=list(v.shape), points=v.numel(), selected=int((v > 0).sum()), components=st[0], largest_root=st[1], largest_size=st[2],
               status=st[3], first_call_ms=first[0], steps=args.steps, warmup=args.warmup)
    if first[0] > args.give_up_ms:
        row["gave_up"] = True
        return row
    again = label()
    row["two_runs_same_bits"] = bool(torch.equal(labels, again[0]) and torch.equal(sizes, again[1]) and torch.equal(stats, again[2]))
    row["label_ms"] = median_ms(label, args.warmup, args.steps)
    row["keep_ms"] = median_ms(keep, args.warmup, args.steps)
    row["points_per_s"] = round(row["points"] / (row["label_ms"][0] * 1e-3))
    t_lab, sweeps, done = torch_labels(v, 8)                                      # warm-up: allocator and kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t_lab, sweeps, done = torch_labels(v, args.max_sweeps)
    torch.cuda.synchronize()
    row["torch_ms"], row["torch_sweeps"], row["torch_converged"] = round((time.perf_counter() - t0) * 1e3, 2), sweeps, done
    if done:
        row["torch_same_labels"] = bool(torch.equal(t_lab, labels))
    del t_lab
    try:
        import numpy as np
        from scipy import ndimage
    except ImportError:
        return row
    structure = np.zeros((3, 3, 3), int)
    structure[1, 1, 1] = 1
    for d in KINDS:
        structure[1 + d[0], 1 + d[1], 1 + d[2]] = structure[1 - d[0], 1 - d[1], 1 - d[2]] = 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lab, k = ndimage.label(v.cpu().numpy() > 0, structure=structure)
    back = torch.from_numpy(lab).to(dev)
    torch.cuda.synchronize()
    row["scipy_ms"], row["scipy_components"] = round((time.perf_counter() - t0) * 1e3, 2), int(k)
    del back
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sweeps", type=int, default=1024)
    ap.add_argument("--give-up-ms", type=float, default=3000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.md"))
    ap.add_argument("--notes", default=os.path.join(ROOT, "profiles", "components_kernel.md"),
                    help="a markdown file appended under the table: the kernels' resource table, read from the compiler")
    ap.add_argument("--rows", default=",".join(r.replace(",", ":") for r in ROWS), help="kind:N,... to run")
    ap.add_argument("--one", default=None, help="run one row 'kind,N' in this process and print it")
    args = ap.parse_args()
    if args.one:
        kind, N = args.one.split(",")
        print("ROW " + json.dumps(row_of(kind, int(N), args)), flush=True)
        return
    rows = []
    for one in [r.replace(":", ",") for r in args.rows.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", one, "--steps", str(args.steps), "--warmup", str(args.warmup), "--max-sweeps",
               str(args.max_sweeps), "--give-up-ms", str(args.give_up_ms)]
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
    md = ["# Connected components of a lattice: `cnerf_components_label` / `_filter` (`scripts/components_bench.py`)", "",
          f"1x MI355X (gfx950).  Device events around each call, {args.warmup} warm-up calls, median of {args.steps} calls (min .. max); every row runs in a",
          "process of its own.  Informational: nothing here is gated.  The feature does not exist before this change, so the yardsticks are what a",
          "user would write without it, on the same card and its host.  `DESIGN.md` 3.25 reads the figures.", "",
          "`label` is `ops.connected_components` (three output allocations, the workspace, five launches), `label + filter` is `ops.keep_components`",
          "(one more allocation and launch).  `torch` is minimum-label propagation over the same 14 neighbours until nothing changes, timed once;",
          "`scipy` is `scipy.ndimage.label` with the same structure plus the copies to the host and back, timed once.  Selection `v > 0`, connectivity 14.", "",
          "| lattice | shape | selected | components | largest | label ms | label + filter ms | points / s | torch ms (sweeps) | torch over label | scipy ms | scipy over label | two runs same bits | status |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        shape = " x ".join(str(s) for s in r["shape"])
        if r.get("gave_up"):
            md.append(f"| {r['kind']} | {shape} | {r['selected']:,} | {r['components']:,} | {r['largest_size']:,} | first call {r['first_call_ms']:.1f}: not timed further | | | | | | | | {r['status']} |")
            continue
        torch_cell = f"{r['torch_ms']:.1f} ({r['torch_sweeps']}{'' if r['torch_converged'] else ', NOT converged'})"
        scipy_cell = f"{r['scipy_ms']:.1f}" if "scipy_ms" in r else "-"
        over = lambda ms: f"{ms / r['label_ms'][0]:.0f}x"
        md.append(f"| {r['kind']} | {shape} | {r['selected']:,} | {r['components']:,} | {r['largest_size']:,} | {f3(r['label_ms'])} | {f3(r['keep_ms'])} | "
                  f"{r['points_per_s']:.3g} | {torch_cell} | {over(r['torch_ms'])}{'' if r['torch_converged'] else ' at least'} | {scipy_cell} | "
                  f"{over(r['scipy_ms']) if 'scipy_ms' in r else '-'} | {r['two_runs_same_bits']} | {r['status']} |")
    md += ["", "Beside them, from `profiles/isosurface.md`: `ops.isosurface` of a 256^3 lattice takes 0.43 ms, the 256^3 field queries before it 58.7 ms."]
    if args.notes and os.path.exists(args.notes):
        md += ["", open(args.notes).read().rstrip()]
    md += ["", "## Raw rows", "", "```"] + [json.dumps(r) for r in rows] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(md))


if __name__ == "__main__":
    main()
