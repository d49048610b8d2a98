#!/usr/bin/env python3
"""Time the MSE+Perceptual_noise loss (csrc/vgg_loss.hip) at 256^2 inputs for batch 16 (BASELINE configs[2] per rank) and 32
(the reference's default batch), for each DRS_VGG_IMPL: the validation forward (2B images), forward + backward, per-layer
times of one forward + backward, and the training step (train_diffusion_superres.py:379-396, 128->256, cosine T=1500,
Adam) with MSE and with MSE+Perceptual_noise.  Seeded VGG19 weights (the time does not depend on their values).  Single GPU;
one JSON line per (batch, impl), then the per-layer table."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from diffusionremotesensing_amd import synthetic  # noqa: E402
from diffusionremotesensing_amd.perceptual import (FEATURE_CHANNELS, FEATURE_CONVS, CombinedLoss,  # noqa: E402
                                                   VGGPerceptualLoss)

POOL_AFTER = (1, 3, 7, 11, 15)


def seeded_sd():
    sd, cin = {}, 3
    for k, cout in zip(FEATURE_CONVS, FEATURE_CHANNELS):
        sd[f"features.{k}.weight"] = synthetic.tensor_normal(f"vgg.features.{k}.weight", (cout, cin, 3, 3), 0,
                                                             std=math.sqrt(2.0 / (9 * cin)))
        sd[f"features.{k}.bias"] = synthetic.tensor_normal(f"vgg.features.{k}.bias", (cout,), 0, std=0.05)
        cin = cout
    return sd


def vgg_flops(n, h=224, w=224):
    """Algorithmic FLOPs (2 x MACs) of the 16 convolutions over n images (a data-gradient pass counts the same)."""
    f, cin = 0.0, 3
    for l, cout in enumerate(FEATURE_CHANNELS):
        f += 2.0 * n * h * w * cin * cout * 9
        cin = cout
        if l in POOL_AFTER:
            h, w = h // 2, w // 2
    return f


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="16,32")
    ap.add_argument("--impls", default="mfma_bf16x3,mfma_f32")
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--no-train-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = seeded_sd()
    S = a.image
    tables = []
    for B in [int(b) for b in a.batches.split(",")]:
        x = synthetic.tensor_normal("bench.vgg.x", (B, 3, S, S)).to(dev)
        y = synthetic.tensor_normal("bench.vgg.y", (B, 3, S, S)).to(dev)
        for impl in a.impls.split(","):
            os.environ["DRS_VGG_IMPL"] = impl
            loss = VGGPerceptualLoss(dev, state_dict=sd)
            xg = x.clone().requires_grad_(True)

            def val():
                with torch.no_grad():
                    loss(x, y)

            def fwd_bwd():
                loss(xg, y).backward()
            ms_val = timed(val, a.steps, a.warmup)
            ms_fb = timed(fwd_bwd, a.steps, a.warmup)
            f_val = vgg_flops(2 * B)
            f_fb = f_val + vgg_flops(B)
            rec = {"batch": B, "image": S, "impl": impl, "val_fwd_ms": ms_val, "val_fwd_tflops": f_val / ms_val * 1e-9,
                   "fwd_bwd_ms": ms_fb, "fwd_bwd_tflops": f_fb / ms_fb * 1e-9}
            # per-layer: one profiled forward + backward
            plan = loss._plan(B, S, S)
            lib = plan.lib
            lib.drs_vgg_profile_enable(plan.handle, 1)
            lb = loss(xg, y)
            fwd_rows = _read(lib, plan)
            lb.backward()
            bwd_rows = _read(lib, plan)
            lib.drs_vgg_profile_enable(plan.handle, 0)
            rows = fwd_rows + bwd_rows
            tables.append((B, impl, rows))
            if not a.no_train_step:
                rec["train_step_mse_ms"] = train_step_ms(dev, B, S, torch.nn.MSELoss(), a)
                rec["train_step_mse_perceptual_ms"] = train_step_ms(
                    dev, B, S, CombinedLoss(torch.nn.MSELoss(), loss, weight_first=0.3), a)
            print(json.dumps(rec), flush=True)
            del loss, plan
            torch.cuda.empty_cache()
    for B, impl, rows in tables:
        print(f"\nper-op times, batch {B}, {impl} (one forward of {2 * B} images + backward of {B}):")
        for name, ms, fl in rows:
            tf = f"{fl / ms * 1e-9:7.1f} TF/s" if fl > 0 and ms > 0 else ""
            print(f"  {name:14s} {ms:8.3f} ms  {tf}")


def _read(lib, plan):
    torch.cuda.synchronize()
    out = []
    name = C.create_string_buffer(64)
    ms, fl = C.c_float(), C.c_double()
    for i in range(lib.drs_vgg_profile_num_ops(plan.handle)):
        st = lib.drs_vgg_profile_read(plan.handle, i, name, 64, C.byref(ms), C.byref(fl))
        if st == 0:
            out.append((name.value.decode(), ms.value, fl.value))
    return out


def train_step_ms(dev, B, S, loss_fn, a):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(synthetic.seeded_state_dict(m.state_dict(), 0))
    m = m.to(dev).train()
    m.hip_engine().set_impl("mfma_bf16x3", train_impl="mfma_f32")  # as tools/bench_train.py
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=2,
                  image_size=S, Degradation_type="DownBlur")
    hr = synthetic.tensor_uniform("train.hr", (B, 3, S, S)).to(dev)
    lr = synthetic.tensor_uniform("train.lr", (B, 3, S // 2, S // 2)).to(dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    return timed(lambda: d.train_step(m, opt, loss_fn, lr, hr), a.steps, a.warmup)


if __name__ == "__main__":
    main()
