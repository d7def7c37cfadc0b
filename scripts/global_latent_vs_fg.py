#!/usr/bin/env python3
"""SHORTSIREN (FiLM field on world positions, no feature volume) against SHORTSIREN_FG (the same four FiLM layers on a looked-up
32-channel feature) in one process: the coarse-pass field kernel of a forward render (hipEvent pair around the launch, median over
the timed steps) in the three precisions, and forward + backward with fp16x3 / fp16.  Workload: 128 x 128 rays x (64 + 64) samples,
batch 8, H = 256.  Prints one JSON line; profiles/global_latent.md records a run.

    python scripts/global_latent_vs_fg.py [--batch 8] [--steps 5] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import cnerf_amd  # noqa: F401
from cnerf_amd.generators import ImplicitGenerator3d

FOV, RAY_START, RAY_END = 49.134342641202636, 0.25, 1.95
# (forward precision, backward precision or None = forward only)
ROWS = [("fp32", None), ("fp16x3", None), ("fp16", None), ("fp16x3", "fp16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--img-size", type=int, default=128)
    ap.add_argument("--num-steps", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
    hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
    events = []
    for _ in range(4):
        e = ctypes.c_void_p()
        assert hip.hipEventCreate(ctypes.byref(e)) == 0
        events.append(e.value)
    B, R, S = args.batch, args.img_size, args.num_steps
    torch.manual_seed(0)
    cam = torch.eye(4, device=dev).unsqueeze(0).repeat(B, 1, 1).contiguous()
    cam[:, 2, 3] = -1.0
    gens = {"SHORTSIREN": ImplicitGenerator3d("SHORTSIREN", 512, 3, 4, args.hidden), "SHORTSIREN_FG": ImplicitGenerator3d("SHORTSIREN_FG", 256, 32, 4, args.hidden)}
    inputs = {"SHORTSIREN": torch.randn(B, 512, device=dev, requires_grad=True),
              "SHORTSIREN_FG": (torch.randn(B, 32, 64, 64, 64, device=dev, requires_grad=True), torch.randn(B, 256, device=dev, requires_grad=True))}
    rows = []
    for variant, gen in gens.items():
        gen.to(dev)
        gen.set_device(dev)
        gen.eval()
        for prec, bprec in ROWS:
            gen.siren.precision, gen.siren.backward_precision = prec, bprec or "fp32"
            kern, wall = [], []
            for i in range(args.warmup + args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.set_grad_enabled(bprec is not None):
                    px, dp = gen(inputs[variant], cam, R, FOV, RAY_START, RAY_END, S, True, clamp_mode="relu", nerf_noise=0.0, white_back=True,
                                 _field_events=events)
                    if bprec is not None:
                        gen.zero_grad()
                        (px.square().mean() + dp.mean()).backward()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    wall.append((time.perf_counter() - t0) * 1e3)
                    ms = ctypes.c_float()
                    assert hip.hipEventSynchronize(events[1]) == 0 and hip.hipEventElapsedTime(ctypes.byref(ms), events[0], events[1]) == 0
                    kern.append(ms.value)
            rows.append({"variant": variant, "precision": prec, "backward_precision": bprec, "coarse_field_kernel_ms": statistics.median(kern),
                         "step_ms": statistics.median(wall), "what": "forward + backward" if bprec else "forward"})
            print(rows[-1], file=sys.stderr, flush=True)
    print(json.dumps({"workload": f"{R}x{R} rays x ({S}+{S}) samples, batch {B}, H {args.hidden}", "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
