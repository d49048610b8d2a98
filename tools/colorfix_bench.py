#!/usr/bin/env python3
"""The two colour-correction kernels (csrc/colorfix.hip) at (16, 3, 256, 256) and (1, 3, 2048, 2048), wavelet with L = 5, next
to the torch composition each replaces in the same process: per level `F.pad(mode="replicate")` + a grouped dilated `F.conv2d`
on both tensors for the wavelet, `mean` / `var` and the affine map for AdaIN.  HIP events around --iters calls after a warm-up,
best of --reps windows.  One JSON line per shape: the time of each entry point (AdaIN: its three launches), of each torch
composition, the speed-up, and the share of the HBM rate reached - the time a single read of both inputs and one write of the
output would take at HBM_BPS over the measured time.  The smaller shape (12.6 MB a tensor) fits the last-level cache, the
larger (50.3 MB a tensor) does too: the share says how close the kernel is to a memory-bound one, not where its bytes came from.
Usage: colorfix_bench.py [--iters 100] [--reps 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402

SHAPES = ((16, 3, 256, 256), (1, 3, 2048, 2048))
LEVELS = 5
HBM_BPS = 8.0e12  # the MI355X's HBM3E peak rate


def _events_ms(fn, iters, reps):
    for _ in range(5):
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


def torch_wavelet(sr, guide, levels=LEVELS):
    C = sr.shape[1]
    k = torch.tensor([0.25, 0.5, 0.25], device=sr.device)
    k = torch.outer(k, k).expand(C, 1, 3, 3).contiguous()

    def low(x):
        for i in range(levels):
            d = 2 ** i
            x = F.conv2d(F.pad(x, (d, d, d, d), mode="replicate"), k, dilation=d, groups=C)
        return x
    return (sr - low(sr)) + low(guide)


def torch_adain(sr, guide):
    mean_s, mean_g = sr.mean(dim=(2, 3), keepdim=True), guide.mean(dim=(2, 3), keepdim=True)
    std_s = torch.sqrt(sr.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    std_g = torch.sqrt(guide.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    return (sr - mean_s) / std_s * std_g + mean_g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    for shape in SHAPES:
        guide = torch.rand(shape, generator=gen).to(dev)
        sr = (guide + 0.05 * torch.randn(shape, generator=gen).to(dev) + 0.03).contiguous()
        nbytes = 4 * sr.numel()
        ideal_ms = 1e3 * 3 * nbytes / HBM_BPS
        # the compositions compute what the kernels compute (fp32 against fp32: reordered sums)
        dw = (hip_ops.colorfix_wavelet(sr, guide, LEVELS) - torch_wavelet(sr, guide)).abs().max().item()
        da = (hip_ops.colorfix_adain(sr, guide) - torch_adain(sr, guide)).abs().max().item()
        ms = {"wavelet": _events_ms(lambda: hip_ops.colorfix_wavelet(sr, guide, LEVELS), args.iters, args.reps),
              "adain": _events_ms(lambda: hip_ops.colorfix_adain(sr, guide), args.iters, args.reps),
              "torch_wavelet": _events_ms(lambda: torch_wavelet(sr, guide), max(args.iters // 5, 1), args.reps),
              "torch_adain": _events_ms(lambda: torch_adain(sr, guide), max(args.iters // 5, 1), args.reps)}
        row = {"shape": list(shape), "levels": LEVELS, "tensor_MB": round(nbytes / 1e6, 1), "iters": args.iters,
               "one_read_of_both_one_write_at_hbm_rate_us": round(1e3 * ideal_ms, 2),
               "max_abs_diff_vs_torch": {"wavelet": dw, "adain": da}}
        for k, v in ms.items():
            row[f"{k}_us"] = round(1e3 * v, 2)
        for k in ("wavelet", "adain"):
            row[f"{k}_speedup_over_torch"] = round(ms[f"torch_{k}"] / ms[k], 2)
            row[f"{k}_hbm_share"] = round(ideal_ms / ms[k], 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
