#!/usr/bin/env python3
"""The two launches behind `Diffusion(prediction=, x0_clip=)`, each next to the torch composition it
replaces, in one process, alternated: `hip_ops.noise_v_target` (x_t and the v target of a training batch) against
`hip_ops.noise_images` plus the torch expression of v, and `hip_ops.pred_to_eps_` (v -> eps, unclipped, clipped, and guided with
the clip) against its torch expression.  Shapes: the benchmark's batch 16 x 3 x 256 x 256 and one small one.  HIP events around
--iters back-to-back calls after a warm-up, best of --reps windows.  The bytes are what each launch must move at 4 bytes per
element: two reads and two writes (v target), two reads and one write (conversion), three and one (guided).  The conversion is
also given as a share of one reverse step of bench.py's configuration (UNet forward, noise draw and ancestral update on the
16-image batch), timed here the same way.  One JSON line per shape.  Usage: prediction_bench.py [--iters 200] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops, synthetic  # noqa: E402

SHAPES = [(16, 3, 256, 256), (2, 3, 64, 64)]
T = 1500
HALF_LINE_BPS = 4.4e12  # the rate 64-byte half lines come back at on this chip


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


def _schedule(dev):
    steps = torch.arange(T) / T
    f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
    return (f_t / f_t[0]).to(dev)


def shape_times(dev, shape, iters, reps):
    gen = torch.Generator().manual_seed(0)
    x0, eps, pred, pu = (torch.randn(shape, generator=gen).to(dev) for _ in range(4))
    B = shape[0]
    t = torch.randint(1, T, (B,), generator=gen).to(dev)
    ah = _schedule(dev)
    out = torch.empty_like(pred)
    clip = (0.0, 1.0)

    def v_target():
        return hip_ops.noise_v_target(x0, eps, t, ah)

    def torch_v_target():
        a = torch.sqrt(ah[t]).view(-1, 1, 1, 1)
        b = torch.sqrt(1.0 - ah[t]).view(-1, 1, 1, 1)
        return hip_ops.noise_images(x0, eps, t, ah), a * eps - b * x0

    def to_eps():
        return hip_ops.pred_to_eps_(pred, x0, t, ah, "v", out=out)

    def to_eps_clip():
        return hip_ops.pred_to_eps_(pred, x0, t, ah, "v", clip, out=out)

    def to_eps_clip_guided():
        return hip_ops.pred_to_eps_(pred, x0, t, ah, "v", clip, pred_uncond=pu, cfg_scale=3.0, out=out)

    def torch_to_eps():
        a = torch.sqrt(ah[t]).view(-1, 1, 1, 1)
        s = torch.sqrt(1.0 - ah[t]).view(-1, 1, 1, 1)
        return s * x0 + a * pred

    def torch_to_eps_clip(p=pred):
        a = torch.sqrt(ah[t]).view(-1, 1, 1, 1)
        s = torch.sqrt(1.0 - ah[t]).view(-1, 1, 1, 1)
        return (x0 - a * torch.clamp(a * x0 - s * p, *clip)) / s

    def torch_to_eps_clip_guided():
        return torch_to_eps_clip(torch.lerp(pu, pred, 3.0))

    # the pairs agree before they are timed
    (xa, va), (xb, vb) = v_target(), torch_v_target()
    assert torch.equal(xa, xb) and torch.allclose(va, vb, rtol=1e-5, atol=1e-6)
    for ours, theirs in ((to_eps, torch_to_eps), (to_eps_clip, torch_to_eps_clip), (to_eps_clip_guided, torch_to_eps_clip_guided)):
        got, want = ours().clone(), theirs()
        assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    us = _events_us({"noise_v_target": v_target, "torch_noise_images_plus_v": torch_v_target, "pred_to_eps_v": to_eps,
                     "torch_to_eps_v": torch_to_eps, "pred_to_eps_v_clip": to_eps_clip, "torch_to_eps_v_clip": torch_to_eps_clip,
                     "pred_to_eps_v_clip_guided": to_eps_clip_guided, "torch_to_eps_v_clip_guided": torch_to_eps_clip_guided},
                    iters, reps)
    n = pred.numel()
    nbytes = {"noise_v_target": 16 * n, "pred_to_eps_v": 12 * n, "pred_to_eps_v_clip": 12 * n, "pred_to_eps_v_clip_guided": 16 * n}
    row = {"shape": list(shape), "iters": iters, "reps": reps}
    row.update({k + "_us": round(v, 2) for k, v in us.items()})
    for k, nb in nbytes.items():
        row[k + "_bytes"] = nb
        row[k + "_bytes_at_half_line_rate_us"] = round(1e6 * nb / HALF_LINE_BPS, 2)
        row[k + "_TB_per_s"] = round(nb / (us[k] * 1e-6) / 1e12, 3)
    return row, us


def reverse_step_us(dev, iters, reps):
    """One reverse step of bench.py's configuration: the forward on the 16 x 3 x 256 x 256 batch (LR 128 x 128, x2, cosine
    T = 1500), the noise draw and the ancestral update."""
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    model = Residual_Attention_UNet_superres(3, 3, dev)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).eval()
    engine = model.hip_engine()
    d = Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2, image_size=256,
                  Degradation_type="DownBlur")
    x = synthetic.tensor_normal("bench.x", (16, 3, 256, 256)).to(dev)
    lr = synthetic.tensor_uniform("bench.lr", (16, 3, 128, 128)).to(dev)
    t_rows = hip_ops.timestep_table(T, 16, dev)
    state = {"first": True}

    def step():
        x.copy_(x0)  # (untrained weights: the state would leave the fp16 range of the FL arithmetic within a few steps)
        eps = engine.forward(x, t_rows[700], lr, 2, reuse_cond=not state["first"], check_weights=state["first"])
        state["first"] = False
        hip_ops.sampler_step_(x, eps, torch.randn_like(x), 700, d.alpha, d.alpha_hat, d.beta)
    x0 = x.clone()
    with torch.no_grad():
        us = _events_us({"reverse_step": step}, max(iters // 10, 5), reps)["reverse_step"]
    engine.check_faults()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("prediction_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    step_us = reverse_step_us(dev, args.iters, args.reps)
    for shape in SHAPES:
        row, us = shape_times(dev, shape, args.iters, args.reps)
        if shape == SHAPES[0]:
            row["reverse_step_us"] = round(step_us, 1)
            for k in ("pred_to_eps_v", "pred_to_eps_v_clip", "pred_to_eps_v_clip_guided"):
                row[k + "_share_of_reverse_step"] = round(us[k] / step_us, 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
