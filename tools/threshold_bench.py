#!/usr/bin/env python3
"""Dynamic x0 thresholding next to what it replaces, in one process, alternated: the whole operation
(`hip_ops.pred_to_eps_(..., x0_threshold=0.995)`), its selection alone (`hip_ops.x0_abs_quantile`), the static clip
(`hip_ops.pred_to_eps_(..., x0_clip)`) and the torch composition (x0, abs, kthvalue per image, clamp, scale, back to eps), for a
v network at 16 x 3 x 256 x 256 and 16 x 13 x 256 x 256, with and without guidance, on two inputs: "realistic" (the implied x0
uniform in [lo - 0.3, hi + 0.3]: the top digit of the keys falls into a few dozen bins) and "gaussian" (prediction and state
N(0, 1)).  HIP events around back-to-back calls after a warm-up, best of --reps windows.  The bytes are those the passes move at
4 bytes per element: pass 1 reads pred (pred_uncond) and x and writes x0, passes 2 and 3 read x0, the apply pass reads x0 and x
and writes eps: 32 (36 guided) in all, 20 (24) for the selection, 12 (16) for the static clip.  The operation is also given as a
share of one DDIM step of bench.py's configuration (UNet forward on the 16 x 3 x 256 x 256 batch and the DDIM update), timed
here the same way.  One JSON line per case.  Usage: threshold_bench.py [--iters 200] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops, synthetic  # noqa: E402

SHAPES = [(16, 3, 256, 256), (16, 13, 256, 256)]
T = 1500
CLIP = (0.0, 1.0)
P = 0.995


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


def _schedule(dev):
    steps = torch.arange(T) / T
    f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
    return (f_t / f_t[0]).to(dev)


def case_times(dev, shape, dist, guided, iters, reps):
    gen = torch.Generator().manual_seed(0)
    B = shape[0]
    t = torch.randint(1, T, (B,), generator=gen).to(dev)
    ah = _schedule(dev)
    a = torch.sqrt(ah[t]).view(-1, 1, 1, 1)
    s = torch.sqrt(1.0 - ah[t]).view(-1, 1, 1, 1)
    lo, hi = CLIP
    c, r = (lo + hi) / 2, (hi - lo) / 2
    if dist == "realistic":
        x0 = (torch.rand(shape, generator=gen) * (hi - lo + 0.6) + lo - 0.3).to(dev)
        eps = torch.randn(shape, generator=gen).to(dev)
        x, pred = a * x0 + s * eps, a * eps - s * x0
        pu = pred + 0.05 * torch.randn(shape, generator=gen).to(dev)  # (guided: the implied x0 overshoots a little further)
    else:
        x, pred, pu = (torch.randn(shape, generator=gen).to(dev) for _ in range(3))
    out = torch.empty_like(pred)
    kw = {"pred_uncond": pu, "cfg_scale": 3.0} if guided else {}
    k = hip_ops.threshold_rank(P, pred[0].numel())

    def dyn():
        return hip_ops.pred_to_eps_(pred, x, t, ah, "v", CLIP, out=out, x0_threshold=P, **kw)

    def select():
        return hip_ops.x0_abs_quantile(pred, x, t, ah, "v", CLIP, P, **kw)

    def static():
        return hip_ops.pred_to_eps_(pred, x, t, ah, "v", CLIP, out=out, **kw)

    def torch_dyn():
        p = torch.lerp(pu, pred, 3.0) if guided else pred
        d = a * x - s * p - c
        sc = d.abs().flatten(1).kthvalue(k + 1, dim=1).values.view(-1, 1, 1, 1)
        sc = torch.where(sc > r, sc, torch.full_like(sc, r))  # (s <= r: clamp(d, -r, r) * 1, the static clip)
        q = c + torch.minimum(torch.maximum(d, -sc), sc) * (r / sc)
        return (x - a * q.clamp(lo, hi)) / s

    # the two agree before they are timed, and so do the scales
    got, want = dyn().clone(), torch_dyn()
    assert (got - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    d = a * x - s * (torch.lerp(pu, pred, 3.0) if guided else pred) - c
    want_s = d.abs().flatten(1).kthvalue(k + 1, dim=1).values
    assert torch.allclose(select(), want_s, rtol=1e-5, atol=0)
    us = _events_us({"threshold": (dyn, iters), "select": (select, iters), "static_clip": (static, iters),
                     "torch": (torch_dyn, max(iters // 20, 3))}, reps)
    n = pred.numel()
    extra = 4 if guided else 0
    nbytes = {"threshold": (32 + extra) * n, "select": (20 + extra) * n, "static_clip": (12 + extra) * n}
    row = {"shape": list(shape), "input": dist, "guided": guided, "p": P, "iters": iters, "reps": reps,
           "dynamic_images": int((want_s > r).sum().item())}
    row.update({key + "_us": round(v, 2) for key, v in us.items()})
    for key, nb in nbytes.items():
        row[key + "_bytes"] = nb
        row[key + "_TB_per_s"] = round(nb / (us[key] * 1e-6) / 1e12, 3)
    row["torch_over_threshold"] = round(us["torch"] / us["threshold"], 1)
    return row, us


def ddim_step_us(dev, iters, reps):
    """One DDIM step of bench.py's configuration: the forward on the 16 x 3 x 256 x 256 batch (LR 128 x 128, x2, cosine
    T = 1500) and the DDIM update (eta = 0)."""
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
        hip_ops.ddim_step_(x, eps, None, 700, 600, 0.0, d.alpha_hat)
    x0 = x.clone()
    with torch.no_grad():
        us = _events_us({"ddim_step": (step, max(iters // 10, 5))}, reps)["ddim_step"]
    engine.check_faults()
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("threshold_bench.py measures on a ROCm device: none is visible")
    dev = torch.device("cuda:0")
    step_us = ddim_step_us(dev, args.iters, args.reps)
    for shape in SHAPES:
        for dist in ("realistic", "gaussian"):
            for guided in (False, True):
                row, us = case_times(dev, shape, dist, guided, args.iters, args.reps)
                if shape == SHAPES[0]:
                    row["ddim_step_us"] = round(step_us, 1)
                    row["threshold_share_of_ddim_step"] = round(us["threshold"] / step_us, 4)
                    row["static_clip_share_of_ddim_step"] = round(us["static_clip"] / step_us, 4)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
