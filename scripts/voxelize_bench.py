#!/usr/bin/env python
"""Times of the point-cloud voxeliser (cnerf_voxelize) against a plain torch statement of the same thing, and of the first-hit picture
(cnerf_voxel_first_hit), on one card; writes the table as markdown (informational; no gate).

Voxeliser: 8 clouds x 100,000 points at G = 32 / 64 / 128 over the cube [-0.6, 0.6]^3, for two clouds -- `surface`: points on a sphere
of radius 0.45 with 0.005 of Gaussian noise, the contention of a scanned object (few cells, many points each); `uniform`: points all
over the cube.  Per row, after warm-up, the median (min, max) over `--steps` windows of 10 back-to-back calls (device events around each window, the two
sides alternating window by window), per call, of
  kernel   ops.voxelize as a user calls it (the bytes query, the workspace and output allocations, the clear and both launches inside)
  torch    the statement a user would write without it: clamp, cell index, index_add_ of ones and of the colours, a divide, the
           permute to (B,4,G,G,G)
and whether two runs of each give the same bits.  The two results are compared (largest colour difference, occupancy equality).
First hit: 8 x 128 x 128 pinhole rays x 256 steps over the G = 64 grid of the surface cloud, cameras on the training shell.

    python scripts/voxelize_bench.py [--steps 20] [--warmup 3] [--out profiles/voxelize.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, LENGTH, MARGIN = 8, 100_000, 1.2, 1e-4
RES = (32, 64, 128)
FOV, RAY_START, RAY_END, R, STEPS_PER_RAY = 49.134342641202636, 0.2, 2.0, 128, 256


INNER = 10       # calls inside one pair of events: a timed window of a few milliseconds, not one call of 0.2 ms


def median_ms(fns, warmup, steps):
    """Per function of `fns` the [median, min, max] ms per call over `steps` windows of INNER back-to-back calls.  The functions ALTERNATE
    window by window (a, b, a, b, ...), so that a drift of the clock or a neighbour on the host meets all of them alike."""
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


def torch_voxelize(pcl, G):
    """The same grid in plain torch: float atomics under index_add_, so the colour sums depend on the order of arrival."""
    import torch
    lo = -LENGTH / 2
    p = pcl[..., :3].clamp(lo + MARGIN, lo + LENGTH - MARGIN)
    ijk = ((p - lo) * (G / LENGTH)).floor().long().clamp_(0, G - 1)
    flat = (ijk[..., 2] * G + ijk[..., 1]) * G + ijk[..., 0]                              # [iz, iy, ix]
    flat = (flat + torch.arange(pcl.shape[0], device=pcl.device)[:, None] * G ** 3).reshape(-1)
    acc = torch.zeros((pcl.shape[0] * G ** 3, 4), device=pcl.device)
    src = torch.cat([torch.ones_like(pcl[..., :1]), pcl[..., 3:6].clamp(0, 1)], -1).reshape(-1, 4)
    acc.index_add_(0, flat, src)
    cnt = acc[:, :1]
    out = torch.cat([(cnt > 0).float(), acc[:, 1:] / cnt.clamp(min=1)], 1)
    return out.reshape(pcl.shape[0], G, G, G, 4).permute(0, 4, 1, 2, 3).contiguous()


def clouds(dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    d = torch.randn((B, N, 3), generator=g, device=dev)
    surface = d / d.norm(dim=-1, keepdim=True) * 0.45 + torch.randn((B, N, 3), generator=g, device=dev) * 0.005
    uniform = (torch.rand((B, N, 3), generator=g, device=dev) - 0.5) * LENGTH
    rgb = torch.rand((B, N, 3), generator=g, device=dev)
    return {"surface": torch.cat([surface, rgb], -1).contiguous(), "uniform": torch.cat([uniform, rgb], -1).contiguous()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize.md"))
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20")
    import torch
    import cnerf_amd  # noqa: F401
    from cnerf_amd import ops, voxels
    from cnerf_amd.generators.volumetric_rendering import sample_camera_positions, create_cam2world_matrix
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for name, pcl in clouds(dev).items():
        for G in RES:
            ours = lambda: ops.voxelize(pcl, G, -LENGTH / 2, LENGTH, clip_margin=MARGIN)
            base = lambda: torch_voxelize(pcl, G)
            a, a2, b, b2 = ours(), ours(), base(), base()
            row = dict(part="voxelize", cloud=name, G=G, B=B, n=N, steps=args.steps, warmup=args.warmup,
                       occupied_cells_per_image=int(a[:, 0].sum()) // B,
                       kernel_two_runs_same_bits=bool(torch.equal(a.view(torch.int32), a2.view(torch.int32))),
                       torch_two_runs_same_bits=bool(torch.equal(b.view(torch.int32), b2.view(torch.int32))),
                       occupancy_equal_share=round(float((a[:, 0] == b[:, 0]).float().mean()), 8),
                       max_colour_diff=float((a[:, 1:] - b[:, 1:]).abs().max()))
            del a2, b, b2
            row["kernel_ms"], row["torch_ms"] = median_ms((ours, base), args.warmup, args.steps)
            row["points_per_s"] = round(B * N / (row["kernel_ms"][0] * 1e-3))
            row["kernel_over_torch"] = round(row["torch_ms"][0] / row["kernel_ms"][0], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    vox = ops.voxelize(clouds(dev)["surface"], 64, -LENGTH / 2, LENGTH, clip_margin=MARGIN)
    cams = create_cam2world_matrix(sample_camera_positions(dev, "y", 0.7, 1.5, B), "y", dev)
    render = lambda: voxels.voxel_surface_render(vox, cams, R, FOV, RAY_START, RAY_END, num_steps=STEPS_PER_RAY, length=LENGTH)
    img = render()
    hit = dict(part="first_hit", B=B, rays_per_image=R * R, num_steps=STEPS_PER_RAY, G=64, steps=args.steps, warmup=args.warmup,
               pixels_lit_share=round(float((img != 1).any(1).float().mean()), 4), two_runs_same_bits=bool(torch.equal(img, render())))
    origins, dirs = voxels.pinhole_rays(cams, R, FOV)
    kernel = lambda: ops.voxel_first_hit(vox, origins, dirs, -LENGTH / 2, LENGTH, RAY_START, RAY_END, STEPS_PER_RAY)
    hit["render_ms"], hit["kernel_ms"] = median_ms((render, kernel), args.warmup, args.steps)
    hit["rays_per_s"] = round(B * R * R / (hit["kernel_ms"][0] * 1e-3))
    print(json.dumps(hit), flush=True)

    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    md = ["# Point-cloud voxeliser and first-hit picture: `cnerf_voxelize`, `cnerf_voxel_first_hit` (`scripts/voxelize_bench.py`)", "",
          f"1x MI355X (gfx950; the runtime names the device \"{torch.cuda.get_device_name(0)}\").  Device events around windows of {INNER} back-to-back calls,",
          f"{args.warmup} warm-up calls, median of {args.steps} windows per call (min .. max); the two sides of a row alternate window by window in one process.",
          "Informational: nothing here is gated.  `DESIGN.md` 3.21 reads the figures.", "",
          f"## Voxeliser: {B} clouds x {N:,} points, cube [-0.6, 0.6]^3, clip margin 1e-4", "",
          "`kernel` is `ops.voxelize` as a user calls it (the bytes query, the workspace and output allocations, the clear and both launches are",
          "inside the timed call).  `torch` is the statement a user would write without it, on the same card in the same process: clamp, cell",
          "index, one `index_add_` of (1, r, g, b) rows, a divide, the permute to (B,4,G,G,G).  `surface`: points on a sphere of radius 0.45 with",
          "0.005 of noise (few cells, many points each); `uniform`: points all over the cube.", "",
          "| cloud | G | occupied cells / image | kernel ms | torch ms | kernel over torch | points / s | kernel: two runs same bits | torch: two runs same bits | max colour difference |",
          "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        md.append(f"| {r['cloud']} | {r['G']} | {r['occupied_cells_per_image']} | {f3(r['kernel_ms'])} | {f3(r['torch_ms'])} | {r['kernel_over_torch']}x | "
                  f"{r['points_per_s']:.3g} | {r['kernel_two_runs_same_bits']} | {r['torch_two_runs_same_bits']} | {r['max_colour_diff']:.3g} |")
    slower = [f"{r['cloud']} G = {r['G']} ({r['kernel_over_torch']}x)" for r in rows if r["kernel_over_torch"] < 1]
    md += ["", f"The kernel took no longer than the torch statement in {len(rows) - len(slower)} of {len(rows)} rows"
           + ("." if not slower else "; it was slower at: " + ", ".join(slower) + ".")]
    md += ["", "The occupancy channels of the two results agreed on a share of "
           + ", ".join(f"{r['occupancy_equal_share']}" for r in rows) + " of the cells (the torch statement rounds the cell coordinate in its own order; nothing is asserted).", "",
           f"## First hit: {B} x {R} x {R} rays x {STEPS_PER_RAY} steps, G = 64 grid of the surface cloud", "",
           "| what | ms | rays / s |", "|---|---|---|",
           f"| `ops.voxel_first_hit` (output allocations inside) | {f3(hit['kernel_ms'])} | {hit['rays_per_s']:.3g} |",
           f"| `voxels.voxel_surface_render` (pinhole rays in torch, the kernel, the permute to (B,3,R,R)) | {f3(hit['render_ms'])} | |", "",
           f"{hit['pixels_lit_share']:.1%} of the pixels hit a voxel; two renders gave the same bits: {hit['two_runs_same_bits']}.", "",
           "## Raw rows", "", "```"] + [json.dumps(r) for r in rows + [hit]] + ["```", ""]
    with open(args.out, "w") as f:
        f.write("\n".join(md))


if __name__ == "__main__":
    main()
