#!/usr/bin/env python3
"""DDIM vs the ancestral chain at BASELINE configs[1]'s shape (superres 128x128 -> 256x256, x2, B = 16, cosine T = 1500),
in one process: wall time of a whole `Diffusion.sample` chain (x_T draw, every forward, update and noise draw, the
fault-word reads) for the DDPM chain (1499 forwards) and DDIM chains with S steps.  One JSON line per chain.
Weights: seeded, with the `output` projection x 1e-2 as in bench.py's `full_chain` (untrained weights make an unbounded
chain, which leaves the FL arithmetic's range and hands the plan over to the split-bf16 kernels mid-run).
Usage: ddim_bench.py [--steps 25,50,100,250] [--eta 0] [--reps 2] [--impl mfma_bf16x3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import synthetic  # noqa: E402
from diffusionremotesensing_amd.train_diffusion_superres import Diffusion  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

BATCH, IMAGE, MAG, T_STEPS = 16, 256, 2, 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="25,50,100,250")
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=2)
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
    d.sample(BATCH, m, lr, sampling_steps=5)  # plan, packed weights and kernels in place before any timing

    def chain_s(S):
        best = float("inf")
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = d.sample(BATCH, m, lr, sampling_steps=S, eta=args.eta)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
            assert torch.isfinite(x).all()
        return best

    ddpm = chain_s(None)
    rows = [("ddpm", T_STEPS - 1, ddpm)] + [("ddim", S, chain_s(S)) for S in (int(s) for s in args.steps.split(",") if s)]
    for kind, S, sec in rows:
        print(json.dumps({"sampler": kind, "steps": S, "eta": args.eta if kind == "ddim" else None,
                          "impl": m.hip_engine().impl, "batch": BATCH, "image": IMAGE, "noise_steps": T_STEPS,
                          "chain_s": round(sec, 4), "images_per_s": round(BATCH / sec, 3),
                          "ms_per_step": round(1e3 * sec / S, 4), "speedup_vs_ddpm": round(ddpm / sec, 2)}), flush=True)


if __name__ == "__main__":
    main()
