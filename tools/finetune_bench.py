#!/usr/bin/env python3
"""Frozen-BatchNorm train plan (DRS_PLAN_FROZEN_BN, `model.freeze_batchnorm()`) against the batch-statistics train plan of
the same build, 128 -> 256 (x2) super-resolution, cosine T = 1500, MSE, FusedAdam.  Single GPU; prints JSON lines.

  --mode steps  (default)  train-step time of the two regimes at every --batch (default 16 and 2): interleaved rounds in one
                           process, median and minimum per-step time of each regime and the ratio of the medians.
  --mode ops               per-op BatchNorm times from the plan profile (drs_unet_profile_*: "<norm>.train" / "<norm>.frozen"
                           forward ops, "<norm>.bwd" backward ops) with their algorithmic bytes: the sums per regime, and the
                           largest layer's backward (reduce + finish + apply against the fused frozen kernel + finish) with
                           the bytes/s each reaches over its own traffic.  Weight gradients run in line for this mode
                           (DRS_WGRAD_STREAM=0) so that nothing overlaps the bracketed kernels.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("steps", "ops"), default="steps")
ap.add_argument("--batch", type=int, nargs="+", default=[16, 2])
ap.add_argument("--image", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=6, help="steps per round and regime")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--iters", type=int, default=5, help="--mode ops: profiled steps per regime")
ap.add_argument("--train-impl", default=os.environ.get("DRS_TRAIN_IMPL", "mfma_f32"))
a = ap.parse_args()
if a.mode == "ops":
    os.environ["DRS_WGRAD_STREAM"] = "0"

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import _lib, synthetic  # noqa: E402
from diffusionremotesensing_amd.optim import FusedAdam  # noqa: E402
from diffusionremotesensing_amd.train_diffusion_superres import Diffusion  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

assert torch.cuda.is_available(), "finetune_bench needs a ROCm device"
dev = torch.device("cuda:0")


def make(frozen):
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 0))
    m = m.to(dev).train()
    m.hip_engine().set_impl("mfma_bf16x3", train_impl=a.train_impl)
    if frozen:
        m.freeze_batchnorm()
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=2,
                  image_size=a.image, Degradation_type="DownBlur")
    return m, d, FusedAdam(m.parameters(), lr=1e-5)


def timed(run, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def bench_steps(B):
    hr = synthetic.tensor_uniform("train.hr", (B, 3, a.image, a.image)).to(dev)
    lr = synthetic.tensor_uniform("train.lr", (B, 3, a.image // 2, a.image // 2)).to(dev)
    loss_fn = torch.nn.MSELoss()
    runs = {}
    for name, frozen in (("batch_stats", False), ("frozen", True)):
        m, d, opt = make(frozen)
        runs[name] = (lambda m=m, d=d, opt=opt: d.train_step(m, opt, loss_fn, lr, hr), m)
        for _ in range(a.warmup):
            runs[name][0]()
    times = {name: [] for name in runs}
    for _ in range(a.rounds):  # interleaved: both regimes see the same clocks and neighbours
        for name, (run, _) in runs.items():
            times[name].append(timed(run, a.steps))
    for _, m in runs.values():
        m.hip_engine().check_faults()
    out = {"metric": "train_step_s", "batch": B, "image": a.image, "train_impl": a.train_impl, "rounds": a.rounds,
           "steps_per_round": a.steps}
    for name, ts in times.items():
        out[name] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    out["frozen_over_batch_stats"] = out["frozen"]["median"] / out["batch_stats"]["median"]
    print(json.dumps(out), flush=True)


def read_ops(plan):
    lib = plan.lib
    name = C.create_string_buffer(128)
    ms, fl, by = C.c_float(), C.c_double(), C.c_double()
    ops = []
    for i in range(lib.drs_unet_profile_num_ops(plan.handle)):
        _lib.check(lib.drs_unet_profile_read(plan.handle, i, name, 128, C.byref(ms), C.byref(fl), C.byref(by)),
                   "drs_unet_profile_read")
        ops.append((name.value.decode(), ms.value, by.value))
    return ops


def bench_ops(B):
    x = synthetic.tensor_normal("train.x", (B, 3, a.image, a.image)).to(dev)
    lr = synthetic.tensor_uniform("train.lr", (B, 3, a.image // 2, a.image // 2)).to(dev)
    noise = synthetic.tensor_normal("train.noise", (B, 3, a.image, a.image)).to(dev)
    t = synthetic.tensor_randint("train.t", (B,), 1, 1500).to(dev)
    for regime, frozen in (("batch_stats", False), ("frozen", True)):
        m, _, _ = make(frozen)

        def step():
            m.zero_grad(set_to_none=True)
            torch.nn.functional.mse_loss(m(x, t, lr, 2), noise).backward()
            torch.cuda.synchronize()
        for _ in range(2):
            step()
        plan = m.hip_engine()._last_plan
        assert plan.train and plan.frozen == frozen
        _lib.check(plan.lib.drs_unet_profile_enable(plan.handle, 1), "drs_unet_profile_enable")
        acc = {}
        try:
            for _ in range(a.iters):
                step()
                for name, ms, by in read_ops(plan):
                    e = acc.setdefault(name, [0.0, by])
                    e[0] += ms
        finally:
            plan.lib.drs_unet_profile_enable(plan.handle, 0)
        m.hip_engine().check_faults()
        fwd = {k: v for k, v in acc.items() if k.endswith((".train", ".frozen"))}
        bwd = {k: v for k, v in acc.items() if k.endswith(".bwd")}
        big = max(bwd, key=lambda k: bwd[k][1])
        big_ms = bwd[big][0] / a.iters
        print(json.dumps({
            "metric": "batchnorm_ops_ms", "regime": regime, "batch": B, "image": a.image, "iters": a.iters,
            "forward_ops": len(fwd), "forward_ms": sum(v[0] for v in fwd.values()) / a.iters,
            "forward_bytes": sum(v[1] for v in fwd.values()),
            "backward_ops": len(bwd), "backward_ms": sum(v[0] for v in bwd.values()) / a.iters,
            "backward_bytes": sum(v[1] for v in bwd.values()),
            "largest_backward": {"op": big, "ms": big_ms, "bytes": bwd[big][1], "TB_per_s": bwd[big][1] / (big_ms * 1e-3) / 1e12},
        }), flush=True)


for B in a.batch:
    (bench_steps if a.mode == "steps" else bench_ops)(B)
