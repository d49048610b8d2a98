#!/usr/bin/env python3
"""The weighted training loss and its gradient, three ways in one process, alternated: the fused launch
(`losses.DiffusionLoss.loss_and_grad`: `drs_diffusion_loss`, table, sampler weights and bins on), the torch composition it
replaces (gather of the weights, per-image means, weighted mean, backward), and the default path's `nn.MSELoss` forward and
backward (unweighted: what a default run pays).  Shapes: 16 x 3 x 256 x 256 and 16 x 13 x 256 x 256.  HIP events around --iters
back-to-back calls after a warm-up, best of --reps windows.  The bytes are what the fused launch must move: two reads and one
write of 4 bytes per element.  One JSON line per shape.  Usage: loss_bench.py [--iters 200] [--reps 5]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import _lib  # noqa: E402
from diffusionremotesensing_amd.losses import CHUNK, KINDS, DiffusionLoss, LossBins  # noqa: E402

SHAPES = [(16, 3, 256, 256), (16, 13, 256, 256)]
T, NBINS = 1500, 16
HALF_LINE_BPS = 4.4e12  # the rate 64-byte half lines come back at on this chip


def _events_us(fns, iters, reps):
    """Best-of-`reps` time per call of every fn, the windows of the fns alternated."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            best[k] = min(best[k], 1e3 * a.elapsed_time(b) / iters)
    return best


def shape_times(dev, shape, iters, reps):
    gen = torch.Generator().manual_seed(0)
    pred, target = torch.randn(shape, generator=gen).to(dev), torch.randn(shape, generator=gen).to(dev)
    B = shape[0]
    t = torch.randint(1, T, (B,), generator=gen).to(dev)
    table = (torch.rand(T, generator=gen) + 0.05).to(dev)
    sample_w = (0.5 + torch.rand(B, generator=gen)).to(dev)
    fused_fn = DiffusionLoss("MSE", table, LossBins(T, NBINS, dev))
    plain_fn = DiffusionLoss("MSE")
    mse = torch.nn.MSELoss()

    def fused():
        return fused_fn.loss_and_grad(pred, target, t, sample_w)

    def fused_unweighted():
        return plain_fn.loss_and_grad(pred, target)

    # the two launches alone, on buffers allocated once: what the device does, without the wrapper's host side
    lib, n = _lib.load(), pred.numel() // B
    grad, per_image = torch.empty_like(pred), torch.empty(B, dtype=torch.float64, device=dev)
    partials = torch.empty(B * ((n + 3) // CHUNK + 1), dtype=torch.float64, device=dev)
    out, bad_t = torch.empty(2, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    bins = LossBins(T, NBINS, dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = [C.c_void_p(x.data_ptr()) for x in (pred, target, t, table, sample_w, grad, per_image, partials, out, bins.buf, bad_t)]

    def launches_only():
        _lib.check(lib.drs_diffusion_loss(ptr[0], ptr[1], ptr[2], B, n, ptr[3], T, ptr[4], KINDS["MSE"], 1.0, ptr[5], ptr[6],
                                          ptr[7], ptr[8], ptr[9], NBINS, bins.history, 1, ptr[10], stream), "drs_diffusion_loss")

    def torch_weighted():
        p = pred.detach().requires_grad_()
        w = table[t] * sample_w
        loss = (w * ((p - target) ** 2).flatten(1).mean(dim=1)).mean()
        loss.backward()
        return loss, p.grad

    def torch_mse():
        p = pred.detach().requires_grad_()
        loss = mse(p, target)
        loss.backward()
        return loss, p.grad

    # the two weighted paths agree before they are timed
    (la, ga), (lb, gb) = fused(), torch_weighted()
    assert abs(la.item() - lb.item()) <= 1e-5 * abs(lb.item()) and torch.allclose(ga, gb, rtol=1e-5, atol=1e-12)
    us = _events_us({"fused_weighted_binned_launches_only": launches_only, "fused_weighted_binned": fused,
                     "fused_unweighted": fused_unweighted,
                     "torch_gather_means_weighted_mean_backward": torch_weighted, "torch_MSELoss_forward_backward": torch_mse},
                    iters, reps)
    fused_fn.check_faults()
    nbytes = 12 * pred.numel()
    row = {"shape": list(shape), "bytes": nbytes, "iters": iters, "reps": reps,
           "bytes_at_half_line_rate_us": round(1e6 * nbytes / HALF_LINE_BPS, 2)}
    row.update({k + "_us": round(v, 2) for k, v in us.items()})
    for k in ("fused_weighted_binned_launches_only", "fused_weighted_binned", "fused_unweighted"):
        row[k + "_TB_per_s"] = round(nbytes / (us[k] * 1e-6) / 1e12, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("loss_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    for shape in SHAPES:
        print(json.dumps(shape_times(dev, shape, args.iters, args.reps)), flush=True)


if __name__ == "__main__":
    main()
