#!/usr/bin/env python3
"""The raw bits of every output of the loss, metric and no-data launches (csrc/loss.hip, csrc/metrics.hip, csrc/nodata.hip) on
seeded inputs, for comparing two builds of the library: the identity tests compare a masked entry with its unmasked sibling and
pass when both move together, and the float64-oracle tests have tolerances.  Public Python API only, so the same file runs
against any checkout that has the no-data entries.  Shapes: (3,3,37,41) crosses a 4096-element chunk with hw % 4 != 0,
(2,1,16,16) and (2,16,12,28) take the vector path (the latter the 16-band instance), (5,2,11,11) is SSIM's single window.

    loss     MSE / MAE / Huber x unit / weighted-with-bins x gradient / none x unmasked / all-valid / NaN rule / value rule:
             loss, loss_f64, gradient, per_image, valid_counts, the bins buffer
    metrics  metrics_pointwise, ssim_mean and their _nodata siblings, clamp on / off, "noise" and "bright_flat" content, the same
             three maskings
    noise    noise_target_nodata for eps / v / x0 under both rules

The masks hold, per batch size, the special images: fully valid, no valid pixel, only the last pixel, one isolated pixel.
Usage: loss_metrics_bits.py --dump FILE | --compare FILE    (--compare exits 1 and names every output that differs)"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops  # noqa: E402
from diffusionremotesensing_amd.losses import DiffusionLoss, LossBins  # noqa: E402

SHAPES = ((3, 3, 37, 41), (2, 1, 16, 16), (2, 16, 12, 28), (5, 2, 11, 11))
T, DELTA, VALUE = 100, 0.3, 0.25
MASKINGS = ("valid", "nan", "value")  # all pixels valid (NaN rule) | NaN-marked | VALUE in all bands


def nodata_pixels(shape):
    """(B, H, W) bool, True = no-data: seeded blocks and isolated pixels, and per batch size the special images."""
    B, _, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))

    def blocks():
        m = torch.zeros(H, W, dtype=torch.bool)
        for _ in range(3):
            y, x = int(torch.randint(0, H - 2, (1,), generator=g)), int(torch.randint(0, W - 2, (1,), generator=g))
            m[y:y + max(H // 4, 2), x:x + max(W // 3, 2)] = True
        m |= torch.rand(H, W, generator=g) < 0.03
        m[0, 0] = True
        return m

    def one(y, x):
        m = torch.zeros(H, W, dtype=torch.bool)
        m[y, x] = True
        return m
    full, none = torch.zeros(H, W, dtype=torch.bool), torch.ones(H, W, dtype=torch.bool)
    return torch.stack({2: [full, blocks()], 3: [blocks(), none, one(-1, -1)],
                        5: [full, none, one(-1, -1), blocks(), one(H // 2, W // 2)]}[B])


def marked(x, masking, g):
    """x with the no-data pixels of its shape carrying the marker of `masking`, and the `nodata` argument that reads it."""
    if masking == "valid":
        return x, True
    nd = nodata_pixels(tuple(x.shape))[:, None]
    if masking == "value":
        return torch.where(nd, torch.full_like(x, VALUE), x), VALUE
    bands = torch.rand(x.shape, generator=g) < 0.5
    bands[:, 0] |= ~bands.any(dim=1)  # at least one band
    return torch.where(nd & bands, torch.full_like(x, math.nan), x), True


def loss_outputs(dev, out):
    for shape in SHAPES[:3]:
        g = torch.Generator().manual_seed(11 + sum(shape))
        B = shape[0]
        pred, target = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
        t = torch.randint(0, T, (B,), generator=g).to(dev)
        table, sample_w = (torch.rand(T, generator=g) + 0.5).to(dev), (torch.rand(B, generator=g) + 0.5).to(dev)
        # masking -> (mask, target): the no-data elements of the target carry the rule's marker, which must reach no output
        cases = {"unmasked": (None, target), "valid": (torch.ones((B, 1) + shape[2:], dtype=torch.uint8), target)}
        for rule in MASKINGS[1:]:
            cases[rule] = ((~nodata_pixels(shape))[:, None].to(torch.uint8), marked(target.cpu(), rule, g)[0].to(dev))
        for kind in ("MSE", "MAE", "Huber"):
            for weighted in (False, True):
                for masking, (valid, target) in cases.items():
                    bins = LossBins(T, 4, dev) if weighted else None
                    fn = DiffusionLoss(kind, table if weighted else None, bins, delta=DELTA)
                    kw = {} if valid is None else {"valid": valid.to(dev)}
                    args = (pred, target, t, sample_w) if weighted else (pred, target)
                    name = f"loss {shape} {kind} {'weighted' if weighted else 'unit'} {masking}"
                    loss, grad = fn.loss_and_grad(*args, **kw)
                    out[name + " grad: loss"], out[name + " grad: loss_f64"] = loss.clone(), fn.loss_f64.clone()
                    out[name + " grad: gradient"], out[name + " grad: per_image"] = grad, fn.per_image
                    if fn.valid_counts is not None:
                        out[name + " grad: valid_counts"] = fn.valid_counts
                    with torch.no_grad():
                        out[name + " nograd: loss"] = fn(*args, **kw).clone()
                    out[name + " nograd: loss_f64"], out[name + " nograd: per_image"] = fn.loss_f64.clone(), fn.per_image
                    if bins is not None:
                        out[name + ": bins"] = bins.buf.clone()


def metric_outputs(dev, out):
    for shape in SHAPES:
        for content in ("noise", "bright_flat"):
            g = torch.Generator().manual_seed(23 + sum(shape) + len(content))
            if content == "noise":  # uniform in [-0.2, 1.2]: the clamp matters
                sr, clean = (torch.rand(shape, generator=g) * 1.4 - 0.2 for _ in range(2))
            else:
                sr, clean = (0.95 + 0.002 * torch.randn(shape, generator=g) for _ in range(2))
            sr = sr.to(dev)
            for clamp in (True, False):
                name = f"metrics {shape} {content} clamp={clamp}"
                out[name + ": metrics_pointwise"] = hip_ops.metrics_pointwise(sr, clean.to(dev), clamp)
                out[name + ": ssim_mean"] = hip_ops.ssim_mean(sr, clean.to(dev), clamp)
                for masking in MASKINGS:
                    hr, nodata = marked(clean, masking, g)
                    hr = hr.to(dev)
                    out[f"{name} {masking}: metrics_pointwise_nodata"] = hip_ops.metrics_pointwise_nodata(sr, hr, nodata, clamp)
                    out[f"{name} {masking}: ssim_nodata"] = hip_ops.ssim_nodata(sr, hr, nodata, clamp)


def noise_outputs(dev, out):
    alpha_hat = torch.linspace(0.999, 0.001, T).to(dev)
    for shape in SHAPES[:3]:
        g = torch.Generator().manual_seed(37 + sum(shape))
        clean, eps = torch.rand(shape, generator=g) * 0.98 + 0.01, torch.randn(shape, generator=g).to(dev)
        t = torch.randint(1, T, (shape[0],), generator=g).to(dev)
        for masking in MASKINGS[1:]:
            x0, nodata = marked(clean, masking, g)
            for prediction in ("eps", "v", "x0"):
                outs = hip_ops.noise_target_nodata(x0.to(dev), eps, t, alpha_hat, prediction, None if nodata is True else nodata)
                for part, x in zip(("x_t", "target", "valid"), outs):
                    out[f"noise {shape} {masking} {prediction}: {part}"] = x


def main():
    ap = argparse.ArgumentParser()
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--dump", metavar="FILE")
    mode.add_argument("--compare", metavar="FILE")
    args = ap.parse_args()
    dev, out = torch.device("cuda:0"), {}
    loss_outputs(dev, out)
    metric_outputs(dev, out)
    noise_outputs(dev, out)
    out = {k: v.detach().cpu().contiguous() for k, v in out.items()}
    if args.dump:
        torch.save(out, args.dump)
        print(f"loss_metrics_bits: dumped {len(out)} outputs to {args.dump}")
        return 0
    want = torch.load(args.compare)

    def same(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8),
                                                                         b.reshape(-1).view(torch.uint8))
    differ = sorted(k for k in out.keys() | want.keys() if k not in out or k not in want or not same(out[k], want[k]))
    for k in differ:
        print("differs:", k)
    print(f"loss_metrics_bits: {len(out)} outputs compared with {args.compare}, {len(differ)} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
