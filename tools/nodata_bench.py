#!/usr/bin/env python3
"""The no-data launches (csrc/nodata.hip, csrc/loss.hip, csrc/metrics.hip) at B = 16, 256 x 256, C = 1, 3 and 13 with a quarter
of the pixels marked, next to their unmasked siblings on tensors of the same size and next to a torch composition of the same
result (`isnan` / `where` / `sum`), in one process.  HIP events around --iters calls after a warm-up, best of --reps windows;
one JSON line per band count:

    noise    noise_target_nodata (x_t, v target, mask)   | noise_v_target                | where / isnan around it
    loss     DiffusionLoss.loss_and_grad(valid=)         | DiffusionLoss.loss_and_grad   | masked MSE and its gradient in torch
    metrics  metrics_pointwise_nodata + ssim_nodata      | metrics_pointwise + ssim_mean | masked squared error and sums in torch

The masked launches move one byte per pixel more than their siblings' 8 .. 12 C bytes (the loss also counts the mask rows
first, one launch more).  Usage: nodata_bench.py [--iters 200] [--reps 3]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402
from diffusionremotesensing_amd.losses import DiffusionLoss  # noqa: E402

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


def _torch_noise(x0, eps, a, b, fill):
    nd = torch.isnan(x0).any(dim=1, keepdim=True)
    x = torch.where(nd, fill, x0)
    return a * x + b * eps, torch.where(nd, 0.0, a * eps - b * x0), ~nd


def _torch_loss(pred, target, valid):
    d = torch.where(valid, pred - target, 0.0)
    n = valid.sum(dim=(1, 2, 3)) * pred.shape[1]
    per_image = (d * d).sum(dim=(1, 2, 3)) / n
    return per_image.mean(), d * (2.0 / (pred.shape[0] * n)).view(-1, 1, 1, 1)


def _torch_sums(sr, hr):
    valid = ~torch.isnan(hr).any(dim=1, keepdim=True)
    s, h = sr.clamp(0, 1), torch.where(valid, hr, 0.0).clamp(0, 1)
    d = torch.where(valid, s - h, 0.0)
    return (d * d).sum(dim=(2, 3)), h.sum(dim=(2, 3)), valid.sum(dim=(1, 2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    for C in (1, 3, 13):
        clean = torch.rand((B, C, H, W), generator=gen).to(dev)
        nd = torch.zeros((B, 1, H, W), dtype=torch.bool, device=dev)
        nd[:, :, : H // 2, : W // 2] = True  # a quarter of every image
        hr = torch.where(nd & (torch.arange(C, device=dev).view(1, C, 1, 1) == 0), math.nan, clean).contiguous()
        sr = (clean + 0.02 * torch.randn((B, C, H, W), generator=gen).to(dev)).contiguous()
        eps = torch.randn((B, C, H, W), generator=gen).to(dev)
        t = torch.randint(1, 1000, (B,), generator=gen).to(dev)
        alpha_hat = torch.linspace(0.999, 0.001, 1000).to(dev)
        a, b = alpha_hat[t].sqrt().view(B, 1, 1, 1), (1 - alpha_hat[t]).sqrt().view(B, 1, 1, 1)
        valid = (~nd).to(torch.uint8).contiguous()
        ws, ws_nd = hip_ops.metrics_workspace(B, C, H, W, dev), hip_ops.metrics_nodata_workspace(B, C, H, W, dev)
        masked_loss, plain_loss = DiffusionLoss("MSE"), DiffusionLoss("MSE")
        it = (args.iters, args.reps)
        ms = {
            "noise": (_events_ms(lambda: hip_ops.noise_target_nodata(hr, eps, t, alpha_hat, "v"), *it),
                      _events_ms(lambda: hip_ops.noise_v_target(clean, eps, t, alpha_hat), *it),
                      _events_ms(lambda: _torch_noise(hr, eps, a, b, 0.5), *it)),
            "loss": (_events_ms(lambda: masked_loss.loss_and_grad(sr, clean, valid=valid), *it),
                     _events_ms(lambda: plain_loss.loss_and_grad(sr, clean), *it),
                     _events_ms(lambda: _torch_loss(sr, clean, ~nd), *it)),
            "metrics": (_events_ms(lambda: (hip_ops.metrics_pointwise_nodata(sr, hr, True, True, ws_nd),
                                            hip_ops.ssim_nodata(sr, hr, True, True, ws_nd)), *it),
                        _events_ms(lambda: (hip_ops.metrics_pointwise(sr, clean, True, ws), hip_ops.ssim_mean(sr, clean, True, ws)), *it),
                        _events_ms(lambda: _torch_sums(sr, hr), *it)),
        }
        row = {"shape": [B, C, H, W], "tensor_MB": round(4 * clean.numel() / 1e6, 1), "nodata_share": 0.25, "iters": args.iters}
        for k, (masked, sibling, composed) in ms.items():
            row[f"{k}_masked_us"], row[f"{k}_sibling_us"] = round(1e3 * masked, 2), round(1e3 * sibling, 2)
            row[f"{k}_torch_us"] = round(1e3 * composed, 2)
            row[f"{k}_masked_over_sibling"] = round(masked / sibling, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
