#!/usr/bin/env python3
"""Known pixels in the tiler, timed in one process: LR 224x288, patch 128, stride 64, x2 = 12 tiles of 256x256 on a 448x576
scene, cosine T = 1500, seeded weights with the `output` projection x 1e-2 (as tools/tiler_bench.py), a block mask that keeps
about half of the scene.  One JSON line with
  * `blend_step_(known=)` (drs_blend_step_known) against `blend_step_` followed by the torch composition of the select
    (known forward-noised with two multiplications and a sum, then torch.where), for a single-band and a per-band mask;
  * `aggregate_tiles(known=)` (drs_aggregate_tiles_known) against `aggregate_tiles` followed by clamp + torch.where;
  * a whole scene chain with known pixels (DDIM, --sampling_steps levels, eta 0, resample 2, jump 2) in both aggregation
    modes, best of --reps calls, next to the same chain without known pixels and without resampling.
The fused kernels read 4 + 1 bytes per element more than the plain ones and save the launches and passes of the composition;
nothing is claimed beyond what this prints.
Usage: tile_known_bench.py [--reps 2] [--impl mfma_bf16x3] [--sampling_steps 10]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import hip_ops, synthetic  # noqa: E402
from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling  # noqa: E402
from diffusionremotesensing_amd.train_diffusion_superres import Diffusion  # noqa: E402
from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres  # noqa: E402

LR_H, LR_W, PATCH, STRIDE, MAG, T_STEPS = 224, 288, 128, 64, 2, 1500


def _events_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--impl", default=None)
    ap.add_argument("--sampling_steps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m = Residual_Attention_UNet_superres(3, 3, dev)
    sd = synthetic.seeded_state_dict(m.state_dict(), 0)
    sd["output.weight"] = sd["output.weight"] * 1e-2
    sd["output.bias"] = sd["output.bias"] * 1e-2
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    eng = m.hip_engine()
    if args.impl:
        eng.set_impl(args.impl)
    S = PATCH * MAG
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, magnification_factor=MAG,
                  image_size=S, Degradation_type="DownBlur")
    img = synthetic.tensor_uniform("tile_known_bench.lr", (1, 3, LR_H, LR_W)).to(dev)
    tiler = split_aggregation_sampling(img, PATCH, STRIDE, MAG, d, dev)
    n = len(tiler.patches_lr)
    Hs, Ws = LR_H * MAG, LR_W * MAG
    gen = torch.Generator().manual_seed(0)
    coarse = torch.rand((Hs // 32, Ws // 32), generator=gen) < 0.5
    mask1 = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1).to(torch.uint8).to(dev)[None].contiguous()
    mask3 = mask1.expand(3, -1, -1).contiguous()
    known = synthetic.tensor_uniform("tile_known_bench.known", (3, Hs, Ws)).to(dev)

    # the step kernel against its composition
    origins = hip_ops.tile_origins([(i[0], i[2]) for i in tiler.patches_sr_infos], S, Hs, Ws, dev)
    weight = tiler.weight[0, 0].contiguous()
    scene = torch.randn((3, Hs, Ws), device=dev)
    eps = torch.randn((n, 3, S, S), device=dev)
    z = torch.randn((3, Hs, Ws), device=dev)
    t, tp = 700, 650
    ah = d.alpha_hat
    ka, kb = float(ah[tp].double().sqrt()), float((1 - ah[tp].double()).sqrt())
    step = {}
    for name, mask in (("mask1", mask1), ("maskC", mask3)):
        mb = mask.bool()

        def fused():
            hip_ops.blend_step_(scene, eps, origins, weight, z, t, alpha_hat=ah, t_prev=tp, eta=0.0, known=known, known_mask=mask)

        def composed():
            hip_ops.blend_step_(scene, eps, origins, weight, None, t, alpha_hat=ah, t_prev=tp, eta=0.0)
            scene.copy_(torch.where(mb, ka * known + kb * z, scene))
        step[name] = (_events_ms(fused, 50), _events_ms(composed, 50))
        scene.normal_()
    plain_ms = _events_ms(lambda: hip_ops.blend_step_(scene, eps, origins, weight, None, t, alpha_hat=ah, t_prev=tp), 50)

    # the final blend against its composition
    tiles = torch.rand((n, 3, S, S), device=dev)
    org_list = [(i[0], i[2]) for i in tiler.patches_sr_infos]
    mb = mask1.bool()
    agg_fused = _events_ms(lambda: hip_ops.aggregate_tiles(tiles, org_list, weight, Hs, Ws, known=known, known_mask=mask1), 20)
    agg_comp = _events_ms(lambda: torch.where(mb, known.clamp(0, 1), hip_ops.aggregate_tiles(tiles, org_list, weight, Hs, Ws)), 20)
    agg_plain = _events_ms(lambda: hip_ops.aggregate_tiles(tiles, org_list, weight, Hs, Ws), 20)

    # whole chains
    torch.manual_seed(0)
    kept = {"known": known, "known_mask": mask1[0], "resample": 2, "jump": 2}
    for mode in ("final", "per_step"):  # plan, packed weights and kernels in place before any timing
        tiler.aggregation_sampling(sampling_steps=2, aggregation=mode, known=known, known_mask=mask1[0])

    def call_s(mode, **kw):
        best = float("inf")
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tiler.aggregation_sampling(sampling_steps=args.sampling_steps, aggregation=mode, **kw)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
            assert torch.isfinite(out).all()
        return best
    chains = {f"{mode}{'_known' if kw else ''}_s": round(call_s(mode, **kw), 4)
              for mode in ("final", "per_step") for kw in ({}, kept)}
    from diffusionremotesensing_amd.sampling import chain_moves
    moves = chain_moves(T_STEPS, args.sampling_steps, 2, 2)
    print(json.dumps({
        "scene": [Hs, Ws], "tiles": n, "tile": S, "noise_steps": T_STEPS, "sampling_steps": args.sampling_steps, "impl": eng.impl,
        "known_fraction": round(mask1.float().mean().item(), 3),
        "moves_known": {"reverse": sum(mv.t_to < mv.t for mv in moves), "jumps": sum(mv.t_to > mv.t for mv in moves)},
        "blend_step_plain_ms": round(plain_ms, 4),
        "blend_step_known_ms": {k: round(v[0], 4) for k, v in step.items()},
        "blend_step_plus_where_ms": {k: round(v[1], 4) for k, v in step.items()},
        "aggregate_plain_ms": round(agg_plain, 4), "aggregate_known_ms": round(agg_fused, 4),
        "aggregate_plus_where_ms": round(agg_comp, 4), **chains}), flush=True)


if __name__ == "__main__":
    main()
