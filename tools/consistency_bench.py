#!/usr/bin/env python3
"""The in-chain LR projection next to what it stands beside, in one process, alternated: one
`hip_ops.lr_consistent_eps_` at B = 16, C = 3, 256 x 256, m = 2 (DownBlur, radius 0.5, damping 0.01), the torch composition of the
same arithmetic (four `matmul` and the element-wise steps, on the projector's own tensors), the x0 form
(`consistency.project`) and the degradation alone (`consistency.degrade`), and one denoise step of bench.py's configuration -
the UNet forward on the 16 x 3 x 256 x 256 batch and the DDIM update, code this feature does not touch - timed the same way.  HIP
events around back-to-back calls after a warm-up, best of --reps windows.  FLOPs and bytes are computed from the shapes: the four
products of a plane are 2 (w W H + h H w + W w h + H h W) operations; the least traffic reads x and eps and writes eps once (12
bytes per element) next to the observation and the matrices, what the launches move also carries the three intermediates
written and read once each.  One JSON line.  Usage: consistency_bench.py [--iters 200] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import consistency, hip_ops, synthetic  # noqa: E402

SHAPE, M, T = (16, 3, 256, 256), 2, 1500


def _events_us(fns, reps):
    """Best-of-`reps` time per call of every (fn, iters), the windows of the fns alternated."""
    for fn, _ in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    best = {k: float("inf") for k in fns}
    for _ in range(reps):
        for k, (fn, iters) in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            best[k] = min(best[k], 1e3 * a.elapsed_time(b) / iters)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("consistency_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    B, Cn, H, W = SHAPE
    model = Residual_Attention_UNet_superres(Cn, Cn, dev)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    engine = model.hip_engine()
    d = Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=M, image_size=H,
                  Degradation_type="DownBlur")
    op = consistency.SeparableOperator.downblur((H, W), M, 0.5)
    p = op.projector(0.01, dev)
    h, w = op.lr_shape
    x0 = synthetic.tensor_normal("bench.x", SHAPE).to(dev)
    x = x0.clone()
    lr = synthetic.tensor_uniform("bench.lr", (B, Cn, h, w)).to(dev)
    eps0 = synthetic.tensor_normal("bench.eps", SHAPE).to(dev)
    eps = eps0.clone()
    t_rows = hip_ops.timestep_table(T, B, dev)
    t = t_rows[700]
    yt = p.prepare(lr)
    ah = d.alpha_hat
    a, s = float(ah[700].double().sqrt()), float((1.0 - ah[700].double()).sqrt())
    state = {"first": True}

    def step():
        x.copy_(x0)  # (untrained weights: the state would leave the fp16 range of the FL arithmetic within a few steps)
        e = engine.forward(x, t, lr, M, reuse_cond=not state["first"], check_weights=state["first"])
        state["first"] = False
        hip_ops.ddim_step_(x, e, None, 700, 600, 0.0, ah)

    def project_eps():
        eps.copy_(eps0)
        return hip_ops.lr_consistent_eps_(eps, x0, t, ah, yt, p)

    def copy_only():
        eps.copy_(eps0)

    def torch_eps():
        z = (x0 - s * eps0) / a
        r = p.G * (yt - torch.matmul(torch.matmul(p.D_y, z), p.D_x.t()))
        return eps0 - (a / s) * torch.matmul(torch.matmul(p.U_y, r), p.U_x.t())

    got, want = project_eps().clone(), torch_eps()
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    with torch.no_grad():
        us = _events_us({"project_eps+copy": (project_eps, args.iters), "copy": (copy_only, args.iters),
                         "torch": (torch_eps, max(args.iters // 4, 5)),
                         "project": (lambda: consistency.project(x0, lr, p), args.iters),
                         "degrade": (lambda: consistency.degrade(x0, op), args.iters),
                         "ddim_step": (step, max(args.iters // 10, 5))}, args.reps)
    engine.check_faults()
    planes, n = B * Cn, B * Cn * H * W
    flop = 2 * planes * (w * W * H + h * H * w + W * w * h + H * h * W)
    least = 12 * n + 4 * planes * h * w
    moved = least + 8 * planes * (w * H + h * w + W * h)
    us["project_eps"] = us["project_eps+copy"] - us["copy"]
    row = {"shape": list(SHAPE), "m": M, "iters": args.iters, "reps": args.reps, "gflop": round(flop / 1e9, 3),
           "least_MB": round(least / 1e6, 1), "moved_MB": round(moved / 1e6, 1)}
    row.update({k + "_us": round(v, 2) for k, v in us.items()})
    row["project_eps_TFLOP_per_s"] = round(flop / (us["project_eps"] * 1e-6) / 1e12, 2)
    row["project_eps_least_us_at_157TF_8TBs"] = round(max(flop / 157.3e12, least / 8e12) * 1e6, 1)
    row["project_eps_share_of_ddim_step"] = round(us["project_eps"] / us["ddim_step"], 4)
    row["torch_over_project_eps"] = round(us["torch"] / us["project_eps"], 2)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
