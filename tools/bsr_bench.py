#!/usr/bin/env python3
"""One batch (16 x 3 x 256 x 256 HR, m = 2) through the blind-degradation feed (diffusionremotesensing_amd/bsr.py, csrc/
bsr_degrade.hip), op by op, next to the torch composition of each op where one exists (`F.pad(mode="reflect")` + grouped
`F.conv2d`, `F.interpolate`, element-wise noise), next to the DownBlur feed's batch, and next to one training step (MSE) at the
same batch.  HIP events around --iters calls after a warm-up, best of --reps windows; the whole-feed rows also give the wall
time per batch of a free-running loop (what the host pays: recipe draw, kernel tables, the upload, the launches).  JPEG has no
torch counterpart: its time is set against the bytes it moves (12 read + 1.5 written and read again as decoded planes + 12
written per pixel) at the HBM rate.  One JSON line per row.
Usage: bsr_bench.py [--iters 50] [--reps 3] [--no-train]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from diffusionremotesensing_amd import bsr  # noqa: E402
from diffusionremotesensing_amd.degradation import DeviceSuperresFeed  # noqa: E402

N, C, S, M = 16, 3, 256, 2
HBM_BPS = 8.0e12  # the MI355X's HBM3E peak rate


def _events_ms(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def torch_blur(x, kernels):
    n, c, h, w = x.shape
    k = kernels.shape[-1]
    wgt = kernels.flip(1, 2)[:, None].expand(n, c, k, k).reshape(n * c, 1, k, k)
    xp = F.pad(x.reshape(1, n * c, h, w), (k // 2,) * 4, mode="reflect")
    return F.conv2d(xp, wgt, groups=n * c).reshape(n, c, h, w)


def torch_sep(x, taps):
    n, c, h, w = x.shape
    k = taps.numel()
    xp = F.pad(x.reshape(n * c, 1, h, w), (k // 2,) * 4, mode="reflect")
    return F.conv2d(F.conv2d(xp, taps.view(1, 1, 1, k)), taps.view(1, 1, k, 1)).reshape(n, c, h, w)


def torch_usm(x, taps):
    b = torch_sep(x, taps)
    soft = torch_sep(((x - b).abs() * 255 > 10).float(), taps)
    return soft * (x + 0.5 * (x - b)).clamp(0, 1) + (1 - soft) * x


def torch_noise(x, z, A):
    return (x + torch.einsum("nij,njhw->nihw", A, z)).clamp(0, 1)


def row(name, ms, **more):
    print(json.dumps({"row": name, "us": round(1e3 * ms, 1), **more}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    u8 = (torch.rand((64, C, S, S), generator=gen) * 255).to(torch.uint8).to(dev)
    x = (u8[:N].float() / 255).contiguous()
    lr = x[:, :, ::M, ::M].contiguous()
    it, rp = args.iters, args.reps
    tensor_mb = 4 * x.numel() / 1e6

    taps = bsr.usm_taps()
    tapd = torch.from_numpy(taps).to(dev)
    d = (bsr.sharpen(x) - torch_usm(x, tapd)).abs().max().item()
    row("sharpen (USM, 51 taps) 256x256", _events_ms(lambda: bsr.sharpen(x), it, rp), tensor_MB=tensor_mb,
        torch_us=round(1e3 * _events_ms(lambda: torch_usm(x, tapd), max(it // 5, 1), rp), 1), max_abs_diff_vs_torch=d)
    rng = np.random.default_rng(0)
    for k, ksize in ((25, None), (25, "drawn"), (7, None)):
        op = bsr._draw_blur(rng, N, M)
        if ksize is None:
            kern = torch.from_numpy(np.stack([bsr.isotropic_gaussian(k, 0.4 * k / 3 + 0.1 * i) for i in range(N)]).astype(np.float32)).to(dev)
            sizes = None
        else:
            kern, sizes = torch.from_numpy(op["kernels"]).to(dev), torch.from_numpy(op["ksize"]).to(dev)
        d = (bsr.blur(x, kern, sizes) - torch_blur(x, kern)).abs().max().item()
        row(f"blur {kern.shape[1]}x{kern.shape[1]} table, sizes {'all ' + str(k) if sizes is None else op['ksize'].tolist()} 256x256",
            _events_ms(lambda: bsr.blur(x, kern, sizes), it, rp),
            torch_us=round(1e3 * _events_ms(lambda: torch_blur(x, kern), max(it // 5, 1), rp), 1), max_abs_diff_vs_torch=d)
    for mode, name in ((1, "bilinear"), (2, "bicubic"), (3, "area")):
        for size in ((S // M, S // M), (int(1.6 * S), int(1.6 * S))):
            kw = {"align_corners": False} if mode != 3 else {}
            if mode == 3 and size[0] > S:
                continue  # (area enlarging is bilinear here; F.interpolate's "area" is adaptive pooling: not the same map)
            d = (bsr.resize(x, size[0], size[1], mode) - F.interpolate(x, size=size, mode=name, **kw).clamp(0, 1)).abs().max().item()
            row(f"resize {name} 256 -> {size[0]}", _events_ms(lambda: bsr.resize(x, size[0], size[1], mode), it, rp),
                torch_us=round(1e3 * _events_ms(lambda: F.interpolate(x, size=size, mode=name, **kw).clamp(0, 1), it, rp), 1),
                max_abs_diff_vs_torch=d)
    nop = bsr._draw_noise(rng, N, C, speckle=False)
    nop["branch"][:] = bsr.BRANCH_CORR
    mode, par = (torch.from_numpy(a).to(dev) for a in bsr.noise_params(nop))
    z = torch.randn(x.shape, device=dev)
    A = par[:, 1:].view(N, 3, 3).contiguous()
    d = (bsr.noise_(x.clone(), z, mode, par) - torch_noise(x, z, A)).abs().max().item()
    work = x.clone()
    row("noise (correlated, in place) 256x256", _events_ms(lambda: bsr.noise_(work, z, mode, par), it, rp),
        torch_us=round(1e3 * _events_ms(lambda: torch_noise(x, z, A), it, rp), 1), max_abs_diff_vs_torch=d,
        randn_us=round(1e3 * _events_ms(lambda: torch.randn(x.shape, device=dev), it, rp), 1))
    q = torch.from_numpy(rng.integers(30, 96, N).astype(np.int32)).to(dev)
    for t, name in ((lr, "128x128"), (x, "256x256")):
        ms = _events_ms(lambda: bsr.jpeg(t, q), it, rp)
        nbytes = t.shape[0] * t.shape[2] * t.shape[3] * 27
        row(f"jpeg {name}", ms, bytes_moved_MB=round(nbytes / 1e6, 2), at_hbm_rate_us=round(1e6 * nbytes / HBM_BPS, 2),
            hbm_share=round(1e3 * nbytes / HBM_BPS / ms, 4))

    feeds = {"bsr plus": bsr.DeviceBSRFeed(u8, M, N, True, "plus", 0), "bsr soft": bsr.DeviceBSRFeed(u8, M, N, True, "soft", 0),
             "downblur": DeviceSuperresFeed(u8, M, 0.5, N, True)}
    feed_ms = {}
    for name, feed in feeds.items():
        for _ in feed:  # warm-up epoch (4 batches)
            pass
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        count = 0
        for _ in range(max(it // 4, 2)):
            for _ in feed:
                count += 1
        host = time.perf_counter() - t0
        b.record()
        torch.cuda.synchronize()
        feed_ms[name] = a.elapsed_time(b) / count
        row(f"feed {name}: one batch", feed_ms[name], host_wall_us_per_batch=round(1e6 * host / count, 1), batches=count)
    if args.no_train:
        return
    from diffusionremotesensing_amd import train_diffusion_superres as T
    from diffusionremotesensing_amd.optim import FusedAdam
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    torch.manual_seed(0)
    model = Residual_Attention_UNet_superres(C, C, dev).to(dev)
    diff = T.Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=M, image_size=S,
                       Degradation_type="BSRGAN")
    opt, loss = FusedAdam(model.parameters(), lr=3e-4), torch.nn.MSELoss()
    model.train()
    batch = next(iter(feeds["bsr plus"]))
    step_ms = _events_ms(lambda: diff.train_step(model, opt, loss, batch[0], batch[1]), 10, 2)
    row("training step (MSE), batch 16, 256x256", step_ms, **{f"feed_{k.replace(' ', '_')}_share_of_step": round(v / step_ms, 4)
                                                              for k, v in feed_ms.items()})


if __name__ == "__main__":
    main()
