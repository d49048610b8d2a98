#!/usr/bin/env python3
"""Band-count sweep at BASELINE configs[1]'s shape (superres, B=16, 256 x 256, x2): eval forwards/s for 3, 4, 13 and 16
bands, the training step (forward + MSE + backward) at 13 bands, and the per-op times (HIP events around every op of the
schedule, drs_unet_profile_*) of the band-dependent ops: conv0, the LR branch, decoder stage 2 and `output`.
One JSON line per measurement.  Usage: multispectral_bench.py [--bands 3,4,13,16] [--iters 50] [--impl mfma_bf16x3]"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffusionremotesensing_amd import synthetic  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

OPS = re.compile(r"conv0|lr_branch|output|\.2$|\.2\.|stage2|dec2")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def model_and_inputs(c, dev, B, S, train=False):
    m = Residual_Attention_UNet_superres(c, c, dev)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 0))
    m = m.to(dev)
    m = m.train() if train else m.eval()
    x = synthetic.tensor_normal(f"msb.{c}.x", (B, c, S, S)).to(dev)
    lr = synthetic.tensor_uniform(f"msb.{c}.lr", (B, c, S // 2, S // 2)).to(dev)
    t = torch.full((B,), 700, dtype=torch.int64, device=dev)
    return m, x, lr, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bands", default="3,4,13,16")
    ap.add_argument("--train-bands", type=int, default=13)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--impl", default="mfma_bf16x3")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, S = a.batch, a.image
    for c in [int(v) for v in a.bands.split(",") if v]:
        m, x, lr, t = model_and_inputs(c, dev, B, S)
        m.hip_engine().set_impl(a.impl)
        with torch.no_grad():
            ms = timed(lambda: m(x, t, lr, 2), a.iters, a.warmup)
            rows = m.hip_engine().profile_forward(x, t, lr, 2, iters=5)
        ops = {name: round(t_ms * 1e3, 1) for name, t_ms, _, _ in rows if OPS.search(name)}
        print(json.dumps({"what": "eval", "bands": c, "impl": a.impl, "B": B, "S": S, "ms_per_forward": round(ms, 4),
                          "forwards_per_s": round(1e3 / ms, 2), "op_us": ops}), flush=True)
        m.hip_engine().check_faults()
        del m
    c = a.train_bands
    m, x, lr, t = model_and_inputs(c, dev, B, S, train=True)
    noise = synthetic.tensor_normal(f"msb.{c}.noise", (B, c, S, S)).to(dev)

    def step():
        m.zero_grad(set_to_none=True)
        F.mse_loss(m(x, t, lr, 2), noise).backward()
    ms = timed(step, max(a.iters // 5, 3), 2)
    print(json.dumps({"what": "train", "bands": c, "B": B, "S": S, "ms_per_step": round(ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
