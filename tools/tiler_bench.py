#!/usr/bin/env python3
"""The tiler's two aggregation modes on one scene, in one process: LR 448x576, patch 128, stride 64, x2 = 48 tiles of
256x256 (three full chunks of 16) on an 896x1152 scene, cosine T = 1500, DDIM S = 50 (eta 0), seeded weights with the
`output` projection x 1e-2 (as tools/ddim_bench.py), best of --reps whole calls.  One JSON line with
  * the whole-call time of aggregation="final" and "per_step", their ratio and the time per step;
  * the time of the per-step kernels outside the forwards (3 x gather_tiles + 1 x blend_step_) and their achieved GB/s
    against the bytes they must move (gather: every tile element read and written once; blend: the scene read and written
    once, every tile's eps read once);
  * the share of a 16-tile forward that is the LR-conditioning branch (forward with the branch minus forward reusing it):
    what the per-step mode pays again in every forward when a scene has more than one chunk;
  * informational: for the final mode, the mean absolute disagreement of neighbouring tiles inside their overlaps before
    blending (what the per-step mode removes by construction), next to the mean |tile value|.
Usage: tiler_bench.py [--reps 2] [--impl mfma_bf16x3] [--sampling_steps 50]"""
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

LR_H, LR_W, PATCH, STRIDE, MAG, T_STEPS = 448, 576, 128, 64, 2, 1500


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
    ap.add_argument("--sampling_steps", type=int, default=50)
    args = ap.parse_args()
    S_steps = args.sampling_steps
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
    img = synthetic.tensor_uniform("tiler_bench.lr", (1, 3, LR_H, LR_W)).to(dev)
    tiler = split_aggregation_sampling(img, PATCH, STRIDE, MAG, d, dev)
    n = len(tiler.patches_lr)
    Hs, Ws = LR_H * MAG, LR_W * MAG
    torch.manual_seed(0)
    for mode in ("final", "per_step"):  # plan, packed weights and kernels in place before any timing
        tiler.aggregation_sampling(sampling_steps=2, aggregation=mode)

    def call_s(mode):
        best = float("inf")
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tiler.aggregation_sampling(sampling_steps=S_steps, aggregation=mode)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
            assert torch.isfinite(out).all()
        return best
    final_s, per_step_s = call_s("final"), call_s("per_step")

    # the per-step kernels outside the forwards
    chunk = 16
    origins = hip_ops.tile_origins([(i[0], i[2]) for i in tiler.patches_sr_infos], S, Hs, Ws, dev)
    weight = tiler.weight[0, 0].contiguous()
    scene = torch.randn((3, Hs, Ws), device=dev)
    eps = torch.randn((n, 3, S, S), device=dev)
    x_tiles = torch.empty((chunk, 3, S, S), device=dev)

    def gathers():
        for c0 in range(0, n, chunk):
            hip_ops.gather_tiles(scene, origins, S, out=x_tiles, first=c0, count=chunk)

    def blend():
        hip_ops.blend_step_(scene, eps, origins, weight, None, 700, alpha_hat=d.alpha_hat, t_prev=699)
    gather_ms, blend_ms = _events_ms(gathers, 50), _events_ms(blend, 50)
    gather_bytes = 2 * 4 * eps.numel()
    blend_bytes = 2 * 4 * scene.numel() + 4 * eps.numel()

    # the conditioning branch of one 16-tile forward
    lr16 = torch.cat([p[:1] for p in tiler.patches_lr[:chunk]], dim=0).contiguous()
    x16 = torch.randn((chunk, 3, S, S), device=dev)
    t16 = torch.full((chunk,), 700, dtype=torch.int64, device=dev)
    m.eval()  # (the samplers leave the model in train mode, like the reference)
    with torch.no_grad():
        fwd_full = _events_ms(lambda: eng.forward(x16, t16, lr16, MAG, reuse_cond=False, check_weights=False), 30)
        fwd_reuse = _events_ms(lambda: eng.forward(x16, t16, lr16, MAG, reuse_cond=True, check_weights=False), 30)
    eng.check_faults()

    # informational: how much neighbouring tiles of the final mode disagree inside their overlaps
    tiles = tiler.sample_tiles(sampling_steps=S_steps)
    infos = tiler.patches_sr_infos
    diffs = []
    for a in range(n):
        for b in range(a + 1, n):
            y0, y1 = max(infos[a][0], infos[b][0]), min(infos[a][1], infos[b][1])
            x0, x1 = max(infos[a][2], infos[b][2]), min(infos[a][3], infos[b][3])
            if y0 < y1 and x0 < x1:
                ta = tiles[a][:, y0 - infos[a][0]:y1 - infos[a][0], x0 - infos[a][2]:x1 - infos[a][2]]
                tb = tiles[b][:, y0 - infos[b][0]:y1 - infos[b][0], x0 - infos[b][2]:x1 - infos[b][2]]
                diffs.append((ta - tb).abs().mean().item())
    n_fwd = S_steps * ((n + chunk - 1) // chunk)
    step_ms = 1e3 * per_step_s / S_steps
    print(json.dumps({
        "scene": [Hs, Ws], "tiles": n, "tile": S, "tile_batch": chunk, "noise_steps": T_STEPS, "sampling_steps": S_steps,
        "impl": eng.impl, "forwards_per_call": n_fwd,
        "final_s": round(final_s, 4), "per_step_s": round(per_step_s, 4), "per_step_over_final": round(per_step_s / final_s, 4),
        "final_ms_per_step": round(1e3 * final_s / S_steps, 3), "per_step_ms_per_step": round(step_ms, 3),
        "gather_ms_per_step": round(gather_ms, 4), "gather_GBps": round(gather_bytes / gather_ms / 1e6, 1),
        "blend_ms_per_step": round(blend_ms, 4), "blend_GBps": round(blend_bytes / blend_ms / 1e6, 1),
        "outside_forwards_share": round((gather_ms + blend_ms) / step_ms, 4),
        "eps_buf_MB": round(4 * eps.numel() / 1e6, 1),
        "forward16_ms": round(fwd_full, 4), "forward16_reuse_cond_ms": round(fwd_reuse, 4),
        "cond_branch_share": round((fwd_full - fwd_reuse) / fwd_full, 4),
        "final_overlap_disagreement_mean_abs": round(sum(diffs) / len(diffs), 5), "overlapping_pairs": len(diffs),
        "final_tile_mean_abs": round(tiles.abs().mean().item(), 5)}), flush=True)


if __name__ == "__main__":
    main()
