#!/usr/bin/env python3
"""The optimizer step on the super-resolution UNet's real parameter list (176 tensors), four ways in one process, alternated:
the plain update (`drs_adam_multi`), the norm launch (`drs_grad_sumsq_partials`), the clipped update (`drs_adamw_clip_multi`)
- each kernel alone on a fixed pointer table, and the two launches back to back - and the torch composition
(`clip_grad_norm_` + `torch.optim.AdamW`).  Then the whole `step()` calls (host side included: table build and upload) of
`FusedAdam` and `FusedAdamW`.  HIP events around --iters calls after a warm-up, best of --reps windows.  The bytes are what the
kernels must move: 28 per element for an update (g, m, v, p read; m, v, p written), 4 for the norm.
With --train-steps N: the training step of bench.py's `train` workload (batch 16 of 256x256, MSE) for N steps with `FusedAdam`
and with `FusedAdamW(weight_decay=0.01, max_grad_norm=1.0)`, host clock around a synchronised window.
One JSON line each.  Usage: optim_bench.py [--iters 200] [--reps 5] [--train-steps 0]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import _lib, synthetic  # noqa: E402
from diffusionremotesensing_amd.optim import CHUNK, FusedAdam, FusedAdamW  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

HBM_BPS = 8.0e12  # the MI355X's HBM3E peak rate


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


def kernel_times(dev, iters, reps):
    shapes = [tuple(p.shape) for p in Residual_Attention_UNet_superres(3, 3, "cpu").parameters()]
    gen = torch.Generator().manual_seed(0)

    def tensors(scale):
        return [(torch.randn(s, generator=gen) * scale).to(dev) for s in shapes]
    p, g, m, v = tensors(0.1), tensors(1e-2), tensors(1e-3), [t.abs() for t in tensors(1e-4)]
    rows, part0 = [], 0
    for i in range(len(shapes)):
        n = p[i].numel()
        rows.append((p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), n, 10, part0))
        part0 += (n + CHUNK - 1) // CHUNK
    table7 = torch.tensor(rows, dtype=torch.int64).view(-1).to(dev)
    table6 = torch.tensor([r[:6] for r in rows], dtype=torch.int64).view(-1).to(dev)
    partials = torch.zeros(part0, dtype=torch.float64, device=dev)
    stats = torch.zeros(6, dtype=torch.int32, device=dev)
    lib = _lib.load()
    nt, max_n = len(rows), max(r[4] for r in rows)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hyper = (1e-4, 0.9, 0.999, 1e-8)

    def plain():
        _lib.check(lib.drs_adam_multi(C.c_void_p(table6.data_ptr()), nt, max_n, *hyper, stream), "drs_adam_multi")

    def norm():
        _lib.check(lib.drs_grad_sumsq_partials(C.c_void_p(table7.data_ptr()), nt, max_n, C.c_void_p(partials.data_ptr()), stream),
                   "drs_grad_sumsq_partials")

    def clipped():
        _lib.check(lib.drs_adamw_clip_multi(C.c_void_p(table7.data_ptr()), nt, max_n, *hyper, 0.01, 1.0, 1,
                                            C.c_void_p(partials.data_ptr()), part0, C.c_void_p(stats.data_ptr()), stream),
                   "drs_adamw_clip_multi")

    def decay_only():  # no partials: the update kernel without its prologue's sum
        _lib.check(lib.drs_adamw_clip_multi(C.c_void_p(table7.data_ptr()), nt, max_n, *hyper, 0.01, 0.0, 0, None, 0,
                                            C.c_void_p(stats.data_ptr()), stream), "drs_adamw_clip_multi")

    def both():
        norm()
        clipped()

    # whole step() calls on parameters of their own, torch's composition next to them
    def params():
        ps = [torch.nn.Parameter(t.clone()) for t in p]
        for q, gi in zip(ps, g):
            q.grad = gi.clone()
        return ps
    pa, pb, pc = params(), params(), params()
    fused, fused_w = FusedAdam(pa, lr=1e-4), FusedAdamW(pb, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    ref = torch.optim.AdamW(pc, lr=1e-4, weight_decay=0.01)

    def torch_step():
        torch.nn.utils.clip_grad_norm_(pc, 1.0)
        ref.step()
    us = _events_us({"plain_update_kernel": plain, "norm_kernel": norm, "clipped_update_kernel": clipped,
                     "update_kernel_without_partials": decay_only, "norm_then_clipped_update": both,
                     "FusedAdam.step": fused.step, "FusedAdamW.step": fused_w.step,
                     "torch_clip_grad_norm_then_AdamW.step": torch_step}, iters, reps)
    n_elem = sum(r[4] for r in rows)
    row = {"tensors": nt, "elements": n_elem, "chunks": part0, "iters": iters, "reps": reps,
           "update_bytes_at_hbm_rate_us": round(1e6 * 28 * n_elem / HBM_BPS, 2),
           "norm_bytes_at_hbm_rate_us": round(1e6 * 4 * n_elem / HBM_BPS, 2)}
    row.update({k + "_us": round(t, 2) for k, t in us.items()})
    row["plain_update_bytes_per_s"] = round(28 * n_elem / (us["plain_update_kernel"] * 1e-6) / 1e12, 3)
    row["unit_of_bytes_per_s"] = "TB/s"
    return row


def train_steps(dev, steps):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    out = {"workload": "superres 256x256 train step, batch 16, MSE (bench.py --workload train)", "steps": steps}
    hr = synthetic.tensor_uniform("train.hr", (16, 3, 256, 256), seed=0).to(dev)
    lr = synthetic.tensor_uniform("train.lr", (16, 3, 128, 128), seed=0).to(dev)
    for name in ("FusedAdam", "FusedAdamW_clip1.0_decay0.01", "FusedAdam_again"):
        m = Residual_Attention_UNet_superres(3, 3, dev)
        m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 0))
        m = m.to(dev).train()
        d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=2,
                      image_size=256, Degradation_type="DownBlur")
        opt = (FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0) if "AdamW" in name
               else FusedAdam(m.parameters(), lr=1e-4))
        loss_fn = torch.nn.MSELoss()
        for _ in range(10):
            d.train_step(m, opt, loss_fn, lr, hr)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            d.train_step(m, opt, loss_fn, lr, hr)
        torch.cuda.synchronize()
        out[name + "_train_steps_per_s"] = round(steps / (time.perf_counter() - t0), 3)
        m.hip_engine().check_faults()
        if "AdamW" in name:
            out["skipped_steps"] = opt.skipped_steps()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps(kernel_times(dev, args.iters, args.reps)), flush=True)
    if args.train_steps:
        print(json.dumps(train_steps(dev, args.train_steps)), flush=True)


if __name__ == "__main__":
    main()
