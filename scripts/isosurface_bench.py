#!/usr/bin/env python3
"""Times of the isosurface stage (cnerf_isosurface_count / _emit) and of the field queries that feed it (informational; no gate).

  ball N     r^2 - |x - c|^2 on an N^3 lattice (N = 128, 256), radius 0.35 of the cube: device events around `count` and around `emit`
             separately (through ctypes, the buffers allocated beforehand), warm-up, median of --steps >= 10.  With the times: the vertex and
             triangle counts, the bytes each pass has to move (a model computed from the shapes: the lattice once, the 9 B per point of
             workspace, the block sums, the outputs) and that over time as a share of the 8 TB/s HBM peak.
  mesh       extract_mesh's two stages at 256^3 on the benchmark's generator (SHORTSIREN_FG, H = 256, 64^3 volume, fp32), timed apart: the
             field queries that fill the grid, and ops.isosurface on it (both entries, the copy of the counts and the allocations
             included), at the median of the grid so that the surface is not empty.  A randomly initialised field has a far larger
             surface than a trained shape: the row is the stage's cost at that size, not at a car's.
  host       the NumPy oracle (tests/isosurface_common.py) on the same 128^3 ball lattice: wall time on the host CPU.  It is the only
             comparison there is -- the capability is new, so there is no earlier time -- and it is a different machine and a different
             program, labelled as such.

Every part runs in a child process of its own under a time limit; the first child that fails ends the run.

    python scripts/isosurface_bench.py [--steps 12] [--warmup 3] [--out profiles/isosurface_rows.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_HBM_GBPS = 8000.0
CHILD_TIMEOUT_S = 240
BALL_RADIUS, CUBE = 0.35, 1.2
PARTS = ("ball128", "ball256", "mesh256", "host128")


def ball_lattice(N, dev=None):
    """Values of the ball field on the N^3 lattice of the cube [-CUBE/2, CUBE/2]^3 (torch on `dev`, or NumPy when dev is None)."""
    pitch = CUBE / (N - 1)
    lo = (-CUBE / 2,) * 3
    if dev is None:
        import isosurface_common as IC
        return IC.ball_field((N, N, N), [(0.01, -0.02, 0.03)], BALL_RADIUS * CUBE, lo, pitch), lo, pitch
    import torch
    ax = torch.arange(N, device=dev, dtype=torch.float32) * pitch + lo[0]
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v = (BALL_RADIUS * CUBE) ** 2 - ((x - 0.01) ** 2 + (y + 0.02) ** 2 + (z - 0.03) ** 2)
    return v.contiguous(), lo, pitch


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
    return sorted(ms)[len(ms) // 2], min(ms), max(ms)


def child_ball(N, args):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, _lib as L
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = L.lib()
    v, lo, pitch = ball_lattice(N, dev)
    nb = C.c_size_t(0)
    L.check(lib.cnerf_isosurface_bytes(N, N, N, C.byref(nb)), "bytes")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    count = lambda: L.check(lib.cnerf_isosurface_count(N, N, N, L.ptr(v), 0.0, L.ptr(counts), L.ptr(ws), ops._stream()), "count")
    count()
    nv, nt = counts.tolist()
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    lo3 = (C.c_float * 3)(*lo)
    emit = lambda: L.check(lib.cnerf_isosurface_emit(N, N, N, L.ptr(v), 0.0, lo3, pitch, None, 0, nv, nt, L.ptr(verts), None, L.ptr(tris), L.ptr(ws),
                                                     ops._stream()), "emit")
    t_count, t_emit = median_ms(count, args.warmup, args.steps), median_ms(emit, args.warmup, args.steps)
    n = N ** 3
    blocks = -(-n // 256)
    # what each pass has to move: count reads the lattice once (the seven neighbour loads are served by the caches) and writes the workspace;
    # emit reads the workspace and writes the mesh (its reads of values and of neighbours' offsets happen only at the surface: left out)
    count_bytes = 4 * n + 9 * n + 2 * 2 * 4 * blocks + 8
    emit_bytes = 9 * n + 2 * 4 * blocks + 12 * nv + 12 * nt
    row = dict(part=f"ball{N}", lattice=[N, N, N], vertices=nv, triangles=nt, workspace_bytes=nb.value,
               count_ms=round(t_count[0], 4), count_ms_min_max=[round(t_count[1], 4), round(t_count[2], 4)],
               emit_ms=round(t_emit[0], 4), emit_ms_min_max=[round(t_emit[1], 4), round(t_emit[2], 4)],
               count_bytes=count_bytes, emit_bytes=emit_bytes,
               count_gbps=round(count_bytes / t_count[0] / 1e6, 1), emit_gbps=round(emit_bytes / t_emit[0] / 1e6, 1), steps=args.steps, warmup=args.warmup)
    row["count_frac_hbm_peak"] = round(row["count_gbps"] / PEAK_HBM_GBPS, 4)
    row["emit_frac_hbm_peak"] = round(row["emit_gbps"] / PEAK_HBM_GBPS, 4)
    print(json.dumps(row), flush=True)


def child_mesh(N, args):
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, extract_shapes as X
    from cnerf_amd.generators import ImplicitGenerator3d
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, 256).to(dev)
    gen.set_device(dev)
    gen.eval()
    z = (torch.randn(1, 32, 64, 64, 64, device=dev), torch.randn(1, 256, device=dev))
    pts, corner, pitch = X.create_samples(N, cube_length=CUBE)
    pts = pts.to(dev)
    field = torch.empty((1, N ** 3, 4), dtype=torch.float32, device=dev)
    max_points = 1 << 22

    def queries():
        with torch.no_grad():
            for s0 in range(0, N ** 3, max_points):
                chunk = pts[:, s0:s0 + max_points].contiguous()
                field[:, s0:s0 + chunk.shape[1]] = gen.siren(chunk, z, N, 1)

    steps = max(args.steps // 2, 5)              # seconds of field work per call: fewer repetitions
    t_field = median_ms(queries, 1, steps)
    grid = field.reshape(N, N, N, 4)
    sigma, rgb = grid[..., 3].contiguous(), grid[..., :3].contiguous()
    level = float(sigma.median())
    lo = (float(corner[2]), float(corner[1]), float(corner[0]))
    surface = lambda: ops.isosurface(sigma, level, lo=lo, pitch=pitch, attrs=rgb)
    v, f, c = ops.isosurface(sigma, level, lo=lo, pitch=pitch, attrs=rgb)
    t_surf = median_ms(surface, args.warmup, args.steps)
    print(json.dumps(dict(part=f"mesh{N}", lattice=[N, N, N], level=level, vertices=len(v), triangles=len(f), field_queries_ms=round(t_field[0], 3),
                          field_queries_ms_min_max=[round(t_field[1], 3), round(t_field[2], 3)], field_steps=steps, isosurface_ms=round(t_surf[0], 3),
                          isosurface_ms_min_max=[round(t_surf[1], 3), round(t_surf[2], 3)], isosurface_over_field=round(t_surf[0] / t_field[0], 4),
                          steps=args.steps, warmup=args.warmup)), flush=True)


def child_host(N, args):
    import isosurface_common as IC
    v, lo, pitch = ball_lattice(N)
    t0 = time.perf_counter()
    verts, faces, _ = IC.isosurface(v, 0.0, lo, pitch)
    dt = time.perf_counter() - t0
    print(json.dumps(dict(part=f"host{N}", lattice=[N, N, N], vertices=len(verts), triangles=len(faces), numpy_oracle_wall_s=round(dt, 3),
                          note="NumPy oracle on the host CPU, one run: another program on another machine, not an earlier version of the kernels")),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parts", default=",".join(PARTS))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.steps >= 10, "median of at least 10 timed calls"
    if args.child:
        kind, N = args.child[:4], int(args.child[4:])
        return {"ball": child_ball, "mesh": child_mesh, "host": child_host}[kind](N, args)
    rows = []
    for part in args.parts.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=CHILD_TIMEOUT_S)      # a child that hangs raises here: nothing more is started
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.exit(f"{part}: child ended with status {p.returncode}; nothing more is started")
        rows += [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
