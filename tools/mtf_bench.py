#!/usr/bin/env python3
"""The sensor-MTF degradation next to what it replaces, in one process, alternated: `hip_ops.fir_decimate`
at 16 x 3 x 256 x 256 and 16 x 13 x 256 x 256, m = 2, g = 0.3 (8 taps per axis), against `hip_ops.sep_apply` with the dense
matrices of the same operator - what the 16-bit feed spends per batch - and against a torch composition (replicate pad and two
strided `conv2d`); and `hip_ops.lr_consistent_eps_` with three distinct band operators against the shared-operator call (the same
launches).  HIP events around back-to-back calls after a warm-up, best of --reps windows; the spread of the windows is reported
beside the best.  Bytes: the least traffic of the FIR reads x and writes out once.  One JSON line.
Usage: mtf_bench.py [--iters 200] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffusionremotesensing_amd import consistency, hip_ops, mtf, synthetic  # noqa: E402

M, G, T = 2, 0.3, 1500


def _events_us(fns, iters, reps):
    """{name: (best, worst)} time per call over `reps` windows of `iters` calls, the windows of the fns alternated."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            seen[k].append(1e3 * a.elapsed_time(b) / iters)
    return {k: (min(v), max(v)) for k, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("mtf_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    out = {"m": M, "nyquist": G, "iters": args.iters, "reps": args.reps}
    taps64, L = mtf.gaussian_taps(G, M)
    taps = torch.from_numpy(taps64).float().to(dev)
    n = taps.numel()
    for bands in (3, 13):
        shape = (16, bands, 256, 256)
        x = synthetic.tensor_uniform("mtf_bench.x", shape).to(dev)
        op = consistency.SeparableOperator.mtf(shape[2:], M, G)
        A_y, A_x = op.matrices(dev)
        ky = taps.view(1, 1, n, 1).expand(bands, 1, n, 1).contiguous()
        kx = taps.view(1, 1, 1, n).expand(bands, 1, 1, n).contiguous()
        pad = (L, n - M - L, L, n - M - L)

        def torch_form():
            p = F.pad(x, pad, mode="replicate")
            return F.conv2d(F.conv2d(p, kx, stride=(1, M), groups=bands), ky, stride=(M, 1), groups=bands)
        fir = hip_ops.fir_decimate(x, taps, taps, L, M)
        assert tuple(torch_form().shape) == tuple(fir.shape) and float((torch_form() - fir).abs().max()) < 1e-5
        assert float((hip_ops.sep_apply(x, A_y, A_x) - fir).abs().max()) < 1e-5
        us = _events_us({"fir_decimate": lambda: hip_ops.fir_decimate(x, taps, taps, L, M),
                         "dense_sep_apply": lambda: hip_ops.sep_apply(x, A_y, A_x), "torch_pad_conv2d": torch_form}, args.iters, args.reps)
        moved = 4 * (x.numel() + fir.numel())
        out[f"16x{bands}x256x256"] = {
            **{k: {"best_us": round(v[0], 2), "worst_us": round(v[1], 2)} for k, v in us.items()}, "taps_per_axis": n,
            "fir_bytes": moved, "fir_tb_per_s": round(moved / us["fir_decimate"][0] / 1e6, 3),
            "dense_over_fir": round(us["dense_sep_apply"][0] / us["fir_decimate"][0], 2),
            "torch_over_fir": round(us["torch_pad_conv2d"][0] / us["fir_decimate"][0], 2)}
    # the in-chain projection: one shared operator against three distinct band operators
    shape = (16, 3, 256, 256)
    shared = consistency.SeparableOperator.mtf(shape[2:], M, G).projector(0.01, dev)
    banded = consistency.BandOperator.mtf(shape[2:], M, (0.35, 0.3, 0.26)).projector(0.01, dev)
    x = synthetic.tensor_normal("mtf_bench.state", shape).to(dev)
    eps0 = synthetic.tensor_normal("mtf_bench.eps", shape).to(dev)
    eps = eps0.clone()
    lr = synthetic.tensor_uniform("mtf_bench.lr", (16, 3, 128, 128)).to(dev)
    t = hip_ops.timestep_table(T, 16, dev)[700]
    ah = torch.cumprod(1.0 - torch.linspace(1e-4, 0.02, T), 0).to(dev)
    yts, ytb = shared.prepare(lr), banded.prepare(lr)

    def project(p, yt):
        eps.copy_(eps0)  # (the call is in place: every call projects the same prediction)
        hip_ops.lr_consistent_eps_(eps, x, t, ah, yt, p)
    us = _events_us({"shared": lambda: project(shared, yts), "three_bands": lambda: project(banded, ytb),
                     "copy_alone": lambda: eps.copy_(eps0)}, args.iters, args.reps)
    out["lr_consistent_eps_16x3x256x256"] = {k: {"best_us": round(v[0], 2), "worst_us": round(v[1], 2)} for k, v in us.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
