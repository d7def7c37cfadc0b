#!/usr/bin/env python3
"""ImplicitGenerator3d.forward against ImplicitGenerator3d.render_rays on the same grid's rays (informational; no gate).

Batch 8, 128 x 128 rays x (64 + 64) samples, SHORTSIREN_FG at H = 256 on a 64^3 volume: the forward in fp32 and fp16x3, forward +
backward in fp16x3 / fp16.  Device events around every step, after warm-up, the two paths alternating inside one loop; one JSON line
per configuration.  --grid-only times forward alone, so that the same script run from a checkout of the parent commit (which has no
render_rays) gives the number to put beside these.

    python scripts/time_render_rays.py [--batch 8] [--steps 8] [--warmup 2] [--grid-only] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import cnerf_amd  # noqa: E402,F401
from cnerf_amd.generators import ImplicitGenerator3d  # noqa: E402

FOV, RAY_START, RAY_END = 49.134342641202636, 0.25, 1.95


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=128)
    ap.add_argument("--num-steps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grid-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, R, S = args.batch, args.img_size, args.num_steps
    gen = ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, 256).to(dev)
    gen.set_device(dev)
    gen.eval()
    gen.rng_mode = "philox"               # no RNG kernels in either path
    fvol = torch.randn(B, 32, 64, 64, 64, device=dev, requires_grad=True)
    glob = torch.randn(B, 256, device=dev, requires_grad=True)
    cam = torch.eye(4, device=dev).unsqueeze(0).repeat(B, 1, 1)
    cam[:, 2, 3] = -1.0
    kw = dict(clamp_mode="relu", nerf_noise=1.0, white_back=True)
    paths = {"forward": lambda: gen((fvol, glob), cam, R, FOV, RAY_START, RAY_END, S, True, **kw)}
    if not args.grid_only:
        from cnerf_amd.generators.volumetric_rendering import pinhole_rays
        origins, dirs = pinhole_rays(cam, R, FOV)
        paths["render_rays"] = lambda: gen.render_rays((fvol, glob), origins, dirs, RAY_START, RAY_END, S, True, **kw)

    lines = []
    for precision, bprec, backward in (("fp32", "fp32", False), ("fp16x3", "fp16", False), ("fp16x3", "fp16", True)):
        gen.siren.precision, gen.siren.backward_precision = precision, bprec

        def step(run):
            if not backward:
                with torch.no_grad():
                    return run()
            for t in (fvol, glob, *gen.parameters()):
                t.grad = None
            px, dp = run()
            (px.square().mean() + dp.mean()).backward()

        for run in paths.values():
            for _ in range(args.warmup):
                step(run)
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(args.steps):                      # alternating: both paths see the same neighbours on the machine
            for k, run in paths.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(run)
                b.record()
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        line = dict(what="fwd+bwd" if backward else "fwd", precision=precision, backward_precision=bprec if backward else None, batch=B,
                    img_size=R, num_steps=S, steps=args.steps,
                    **{f"{k}_ms": round(sorted(v)[len(v) // 2], 3) for k, v in ms.items()}, **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()})
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
