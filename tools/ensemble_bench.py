#!/usr/bin/env python3
"""The two ensemble kernels (csrc/ensemble.hip) at (N, 16, 3, 256, 256) for N = 4, 8, 16, 32, next to the torch composition
each one replaces, on the same seeded tensors in the same process:

    ensemble_stats   mean, std and three quantile maps     vs  torch.sort + mean + var + the interpolation of the quantiles
    ensemble_scores  per-image sums, rank histogram        vs  torch.sort + the two CRPS sums + mean + var + rank + bincount

HIP events around --iters calls after a warm-up; the two sides alternate over --reps rounds and the best window of each is
reported (the composition gets --iters / 10 calls per window: it is that much slower).  One JSON line per N with the time
of each side and the rate N * elements * 4 bytes / time of the kernels - the bytes of the members, which each kernel reads
once; the maps it writes (5 and 0 element-sized tensors) and the truth are not counted.  The last-level cache holds 256 MB:
the N = 4 and N = 8 members (50 and 101 MB) fit in it, so their rates are not HBM rates.
Usage: ensemble_bench.py [--iters 100] [--reps 3]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402

B, C, H, W = 16, 3, 256, 256
QUANTILES = (0.05, 0.5, 0.95)


def torch_stats(x):
    N = x.shape[0]
    s = torch.sort(x, dim=0).values
    out = [x.mean(dim=0), x.var(dim=0, unbiased=True).sqrt()]
    for q in QUANTILES:
        pos = q * (N - 1)
        k = int(pos)
        out.append(torch.lerp(s[k], s[min(k + 1, N - 1)], pos - k))
    return out


def torch_scores(x, y):
    N = x.shape[0]
    s = torch.sort(x, dim=0).values
    w = (2.0 * torch.arange(N, device=x.device, dtype=x.dtype) - N + 1).view(N, 1, 1, 1, 1)
    crps = (s - y).abs().mean(dim=0) - (w * s).sum(dim=0) / N ** 2
    mean, var = x.mean(dim=0), x.var(dim=0, unbiased=True)
    sums = torch.stack([t.flatten(1).sum(dim=1) for t in (crps, var, (mean - y) ** 2)], dim=1)
    rank = (x < y).sum(dim=0) + (N + 1) * torch.arange(y.shape[0], device=x.device).view(-1, 1, 1, 1)
    return sums, torch.bincount(rank.flatten(), minlength=y.shape[0] * (N + 1))


def _window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    y = torch.rand((B, C, H, W), generator=gen).to(dev)
    for N in (4, 8, 16, 32):
        x = torch.cat([(y + 0.05 * torch.randn((B, C, H, W), generator=gen).to(dev))[None] for _ in range(N)]).contiguous()
        sides = {"stats": lambda: hip_ops.ensemble_stats(x, QUANTILES), "stats_torch": lambda: torch_stats(x),
                 "scores": lambda: hip_ops.ensemble_scores(x, y), "scores_torch": lambda: torch_scores(x, y)}
        iters = {k: max(args.iters // 10, 1) if k.endswith("torch") else args.iters for k in sides}
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        best = {k: float("inf") for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():  # the sides alternate
                best[k] = min(best[k], _window_ms(fn, iters[k]))
        nbytes = 4 * x.numel()
        row = {"members": [N, B, C, H, W], "members_MB": round(nbytes / 1e6, 1), "iters": args.iters}
        for k in ("stats", "scores"):
            row[f"{k}_us"] = round(1e3 * best[k], 2)
            row[f"{k}_GBps"] = round(nbytes / best[k] / 1e6, 1)
            row[f"{k}_torch_us"] = round(1e3 * best[k + "_torch"], 2)
            row[f"{k}_speedup"] = round(best[k + "_torch"] / best[k], 1)
        print(json.dumps(row), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
