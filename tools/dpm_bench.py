#!/usr/bin/env python3
"""DPM-Solver++(2M) vs DDIM at BASELINE configs[1]'s shape (superres 128x128 -> 256x256, x2, B = 16, cosine T = 1500), in one
process: wall time of a whole `Diffusion.sample` chain (x_T draw, the level list's read-back of the schedule, every forward and
update, the fault-word reads) for DDIM chains (uniform levels) and 2M chains (logSNR levels).  One JSON line per chain.
Weights: seeded, with the `output` projection x 1e-2, as in tools/ddim_bench.py.
Usage: dpm_bench.py [--ddim 50,25] [--dpm 20,10] [--reps 3] [--impl mfma_bf16x3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import synthetic  # noqa: E402
from diffusionremotesensing_amd.sampling import sampling_plan  # noqa: E402
from diffusionremotesensing_amd.train_diffusion_superres import Diffusion  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

BATCH, IMAGE, MAG, T_STEPS = 16, 256, 2, 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ddim", default="50,25")
    ap.add_argument("--dpm", default="20,10")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--impl", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = Residual_Attention_UNet_superres(3, 3, dev)
    sd = synthetic.seeded_state_dict(m.state_dict(), 0)
    sd["output.weight"] = sd["output.weight"] * 1e-2
    sd["output.bias"] = sd["output.bias"] * 1e-2
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    if args.impl:
        m.hip_engine().set_impl(args.impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, magnification_factor=MAG,
                  image_size=IMAGE, Degradation_type="DownBlur")
    lr = synthetic.tensor_uniform("ddim_bench.lr", (BATCH, 3, IMAGE // MAG, IMAGE // MAG)).to(dev)
    torch.manual_seed(0)
    for solver in ("ddim", "dpmpp_2m"):  # plan, packed weights and both update kernels in place before any timing
        d.sample(BATCH, m, lr, sampling_steps=sampling_plan(5, solver))

    def chain_s(S, solver):
        best = float("inf")
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = d.sample(BATCH, m, lr, sampling_steps=sampling_plan(S, solver))
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
            assert torch.isfinite(x).all()
        return best

    rows = [("ddim", int(s)) for s in args.ddim.split(",") if s] + [("dpmpp_2m", int(s)) for s in args.dpm.split(",") if s]
    for solver, S in rows:
        sec = chain_s(S, solver)
        print(json.dumps({"sampler": solver, "spacing": "logsnr" if solver == "dpmpp_2m" else "uniform", "steps": S,
                          "impl": m.hip_engine().impl, "batch": BATCH, "image": IMAGE, "noise_steps": T_STEPS,
                          "chain_s": round(sec, 4), "images_per_s": round(BATCH / sec, 3),
                          "ms_per_step": round(1e3 * sec / S, 4)}), flush=True)


if __name__ == "__main__":
    main()
