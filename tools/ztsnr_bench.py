#!/usr/bin/env python3
"""The two launches behind `Diffusion(zero_terminal_snr=True)` and `guidance_rescale`, each next to the
torch composition it stands for, in one process, alternated: `hip_ops.terminal_step_` (the move away from the terminal level: a v
prediction, plain, with the clip and the move's noise, and guided with the clip, noise and the DPM history) and
`hip_ops.cfg_rescale` (phi = 0.7).  Shapes: 16 x 3 x 256 x 256 and 16 x 13 x 256 x 256.  HIP events around --iters back-to-back
calls after a warm-up, best of --reps windows.  The bytes are what each launch must move at 4 bytes per element: the move reads x
and the prediction and writes x (12 n; + 4 n each for the noise, the unconditional prediction and the history); the rescale reads
both predictions twice and writes once (20 n; its partial sums are a few KiB).  One JSON line per shape.
Usage: ztsnr_bench.py [--iters 200] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402
from diffusionremotesensing_amd.sampling import rescale_zero_terminal_snr  # noqa: E402

SHAPES = [(16, 3, 256, 256), (16, 13, 256, 256)]
T = 1500
T_PREV = 1250
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


def _schedule(dev):
    steps = torch.arange(T) / T
    f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
    return rescale_zero_terminal_snr(f_t / f_t[0]).to(dev)


def shape_times(dev, shape, iters, reps):
    gen = torch.Generator().manual_seed(0)
    x0, pred, pu, z = (torch.randn(shape, generator=gen).to(dev) for _ in range(4))
    ah = _schedule(dev)
    x, hist, out = x0.clone(), torch.empty_like(x0), torch.empty_like(x0)
    clip, eta = (0.0, 1.0), 0.5
    ap = float(ah[T_PREV])
    c0, c1, sg = ap ** 0.5, ((1 - ap) * (1 - eta * eta)) ** 0.5, eta * (1 - ap) ** 0.5

    def step():
        return hip_ops.terminal_step_(x, pred, None, T - 1, T_PREV, ah, "v")

    def step_clip_noise():
        return hip_ops.terminal_step_(x, pred, z, T - 1, T_PREV, ah, "v", eta=eta, x0_clip=clip)

    def step_clip_noise_guided_hist():
        return hip_ops.terminal_step_(x, pred, z, T - 1, T_PREV, ah, "v", eta=eta, x0_clip=clip, pred_uncond=pu, cfg_scale=3.0,
                                      hist=hist)

    def torch_step():
        return x.copy_(c0 * (-pred) + (1 - ap) ** 0.5 * x)

    def torch_step_clip_noise(p=pred):
        return x.copy_(c0 * torch.clamp(-p, *clip) + c1 * x + sg * z)

    def torch_step_clip_noise_guided_hist():
        q = torch.clamp(-torch.lerp(pu, pred, 3.0), *clip)
        hist.copy_(q)
        return x.copy_(c0 * q + c1 * x + sg * z)

    def rescale():
        return hip_ops.cfg_rescale(pred, pu, 3.0, 0.7, out=out)

    def torch_rescale():
        g = torch.lerp(pu, pred, 3.0)
        f = 1 + 0.7 * (pred.flatten(1).std(dim=1, unbiased=False) / g.flatten(1).std(dim=1, unbiased=False) - 1)
        return g * f.view(-1, 1, 1, 1)

    # the pairs agree before they are timed
    for ours, theirs in ((step, torch_step), (step_clip_noise, torch_step_clip_noise),
                         (step_clip_noise_guided_hist, torch_step_clip_noise_guided_hist)):
        x.copy_(x0)
        got = ours().clone()
        x.copy_(x0)
        want = theirs().clone()
        assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    got, want = rescale().clone(), torch_rescale()
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()
    us = _events_us({"terminal_step_v": step, "torch_terminal_step_v": torch_step, "terminal_step_v_clip_noise": step_clip_noise,
                     "torch_terminal_step_v_clip_noise": torch_step_clip_noise,
                     "terminal_step_v_clip_noise_guided_hist": step_clip_noise_guided_hist,
                     "torch_terminal_step_v_clip_noise_guided_hist": torch_step_clip_noise_guided_hist,
                     "cfg_rescale": rescale, "torch_cfg_rescale": torch_rescale}, iters, reps)
    n = pred.numel()
    nbytes = {"terminal_step_v": 12 * n, "terminal_step_v_clip_noise": 16 * n, "terminal_step_v_clip_noise_guided_hist": 24 * n,
              "cfg_rescale": 20 * n}
    row = {"shape": list(shape), "iters": iters, "reps": reps}
    row.update({k + "_us": round(v, 2) for k, v in us.items()})
    for k, nb in nbytes.items():
        row[k + "_bytes"] = nb
        row[k + "_bytes_at_half_line_rate_us"] = round(1e6 * nb / HALF_LINE_BPS, 2)
        row[k + "_TB_per_s"] = round(nb / (us[k] * 1e-6) / 1e12, 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ztsnr_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    for shape in SHAPES:
        print(json.dumps(shape_times(dev, shape, args.iters, args.reps)), flush=True)


if __name__ == "__main__":
    main()
