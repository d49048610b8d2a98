#!/usr/bin/env python3
"""The two image-quality kernels (csrc/metrics.hip) at B = 16, 256 x 256, C = 3 and C = 13, next to the project's plain
streaming kernel (drs_noise_images) on tensors of the same size in the same process.  HIP events around --iters calls after
a warm-up, best of --reps windows; one JSON line per band count with the time of each entry point (its fixed-order reduction
launch included) and the achieved GB/s against the bytes it must move (the metrics read two tensors, noise_images reads two
and writes one).  All three run on the same buffers, so whatever the last-level cache holds of them, it holds for each.
Usage: metrics_bench.py [--iters 200] [--reps 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402

B, H, W = 16, 256, 256


def _events_ms(fn, iters, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    for C in (3, 13):
        hr = torch.rand((B, C, H, W), generator=gen).to(dev)
        sr = (hr + 0.02 * torch.randn((B, C, H, W), generator=gen).to(dev)).contiguous()
        t = torch.randint(1, 1000, (B,), generator=gen).to(dev)
        alpha_hat = torch.linspace(0.999, 0.001, 1000).to(dev)
        ws = hip_ops.metrics_workspace(B, C, H, W, dev)
        nbytes = 4 * hr.numel()
        ms = {"pointwise": _events_ms(lambda: hip_ops.metrics_pointwise(sr, hr, True, ws), args.iters, args.reps),
              "ssim": _events_ms(lambda: hip_ops.ssim_mean(sr, hr, True, ws), args.iters, args.reps),
              "noise_images": _events_ms(lambda: hip_ops.noise_images(hr, sr, t, alpha_hat), args.iters, args.reps)}
        moved = {"pointwise": 2 * nbytes, "ssim": 2 * nbytes, "noise_images": 3 * nbytes}
        row = {"shape": [B, C, H, W], "tensor_MB": round(nbytes / 1e6, 1), "iters": args.iters}
        for k in ms:
            row[f"{k}_us"] = round(1e3 * ms[k], 2)
            row[f"{k}_GBps"] = round(moved[k] / ms[k] / 1e6, 1)
        row["pointwise_over_streaming_rate"] = round(row["pointwise_GBps"] / row["noise_images_GBps"], 3)
        row["ssim_over_streaming_rate"] = round(row["ssim_GBps"] / row["noise_images_GBps"], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
