#!/usr/bin/env python3
"""The fused known-pixel move (hip_ops.inpaint_step_) against the composition it replaces, in one process, at the update
shapes of the super-resolution (16, 3, 256, 256) and SAR -> NDVI (16, 1, 128, 128) samplers, DDIM (eta = 1) and ancestral form:

    composition   y = x.clone(); ddim_step_(y, ...) / sampler_step_(y, ...); kn = known * a; kn.add_(z, alpha=b);
                  x = torch.where(mask, kn, y)

Both are timed with device events over `--iters` calls per window, the two alternating window by window (`--reps` windows
each, the median is reported), after a warm-up of both.  Every call works on the next of `sets` independent sets of tensors,
enough of them (>= 768 MB together) that no call finds its operands in the 256 MiB last-level cache: the rates are HBM rates.
Byte model per element (fp32 tensors, a uint8 mask of one band): fused 20 + 1 / C (x, eps, z, known read, x written, the mask);
composition 8 (clone) + 16 (update) + 8 + 12 (forward noising) + 12 + 1 / C (where) = 56 + 1 / C.  One JSON line per row;
the outputs of the two are compared first (same bits on the unknown pixels, <= 1 ulp-level difference on the known ones: the
composition rounds b * z into the sum in one fused step, the kernel does not).
Usage: inpaint_bench.py [--iters 200] [--reps 7]"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops, synthetic  # noqa: E402

T_STEPS, T, T_PREV = 1500, 750, 720
SHAPES = ((16, 3, 256, 256), (16, 1, 128, 128))


def schedule(dev):
    steps = torch.arange(T_STEPS) / T_STEPS
    f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
    ah = f_t / f_t[0]
    beta = torch.empty_like(ah)
    beta[0] = 1 - ah[0]
    beta[1:] = 1 - ah[1:] / ah[:-1]
    return (1.0 - beta).to(dev), ah.to(dev), beta.to(dev)


def time_windows(fns, iters, reps):
    """Median ms per call of every function of `fns`, windows of `iters` calls alternating between them."""
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(iters):
                fn(i)
            stop.record()
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop) / iters)
    return [statistics.median(m) for m in ms], [(min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    alpha, ah, beta = schedule(dev)
    for shape in SHAPES:
        n, C, H, W = shape
        numel = n * C * H * W
        sets = max(2, math.ceil(768e6 / (numel * 20)))
        gen = torch.Generator(device=dev).manual_seed(0)
        masks = [synthetic.block_mask("inpaint_bench.m", n, H, 0.4, H // 8, seed=s).to(dev) for s in range(min(sets, 4))]
        data = [tuple(torch.randn(shape, device=dev, generator=gen) for _ in range(4)) + (masks[s % len(masks)].clone(),)
                for s in range(sets)]
        masks_b = [d[4].bool() for d in data]
        for form in ("ddim", "ancestral"):
            t_prev = T_PREV if form == "ddim" else T - 1
            a, b = math.sqrt(float(ah[t_prev])), math.sqrt(1.0 - float(ah[t_prev]))
            kw = {"t_prev": T_PREV, "eta": 1.0} if form == "ddim" else {"alpha": alpha, "beta": beta}

            def fused(i, x=None):
                xs, e, z, kn, m = data[i % sets]
                return hip_ops.inpaint_step_(xs if x is None else x, e, z, kn, m, T, alpha_hat=ah, **kw)

            def composed(i, keep=True):
                xs, e, z, kn, _ = data[i % sets]
                y = xs.clone()
                if form == "ddim":
                    hip_ops.ddim_step_(y, e, z, T, T_PREV, 1.0, ah)
                else:
                    hip_ops.sampler_step_(y, e, z, T, alpha, ah, beta)
                noised = kn * a
                noised.add_(z, alpha=b)
                out = torch.where(masks_b[i % sets], noised, y)
                if keep:
                    data[i % sets] = (out,) + data[i % sets][1:]  # the chain's state moves on, as with the in-place kernel
                return out
            # same result first (on copies: the timed calls below work in place)
            got, want = fused(0, data[0][0].clone()), composed(0, keep=False)
            mb = masks_b[0].expand_as(got)
            assert torch.equal(got[~mb], want[~mb])
            known_diff = ((got - want).abs().max() / want.abs().max()).item()
            assert known_diff <= 2.4e-7, known_diff
            for fn in (fused, composed):  # warm-up of both, every set touched
                for i in range(sets):
                    fn(i)
            torch.cuda.synchronize()
            (f_ms, c_ms), spread = time_windows((fused, composed), args.iters, args.reps)
            f_bytes, c_bytes = numel * 20 + numel // C, numel * 56 + numel // C
            print(json.dumps({"shape": list(shape), "form": form, "sets": sets, "iters": args.iters, "reps": args.reps,
                              "fused_us": round(1e3 * f_ms, 2), "composed_us": round(1e3 * c_ms, 2),
                              "fused_us_min_max": [round(1e3 * v, 2) for v in spread[0]],
                              "composed_us_min_max": [round(1e3 * v, 2) for v in spread[1]],
                              "speedup": round(c_ms / f_ms, 2),
                              "fused_model_bytes": f_bytes, "composed_model_bytes": c_bytes,
                              "fused_GBps": round(f_bytes / f_ms / 1e6, 1), "composed_GBps": round(c_bytes / c_ms / 1e6, 1),
                              "known_max_rel_diff": known_diff}), flush=True)
        del data, masks_b
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
