#!/usr/bin/env python3
"""The three launches of csrc/radiometry.hip next to what each replaces, in one process:
  crop       16 items x 13 bands, 256 x 256 windows of 512 x 512 uint16 scenes -> normalised fp32 (+ the NaN-marked copy):
             drs_crop_d4_u16_f32 against the torch composition (per item index, slice, flip / transpose, stack, convert,
             normalise) and against the 8-bit sibling drs_crop_d4_u8_f32 on a uint8 cache of the same shape and items (bytes/s);
  histogram  16 scenes x 13 bands x 512 x 512: drs_hist_u16 against torch.bincount per band (convert + 13 calls), on uniform
             values, on scene-like values (a gamma law: a few hundred values carry a band) and on constant planes;
  quantize   16 x 13 x 256 x 256 fp32 -> uint16: drs_quantize_u16 against clamp, multiply, add, round, clamp, where, cast.
The crop's caches are larger than the Infinity Cache (--scenes scenes) and every call takes the next batch of seeded items,
uploaded before the clock starts.  HIP events around --iters calls after a warm-up; --reps windows per entry, the entries taking
turns; one JSON line per row with min / median / max of the window means.  Before timing, each launch is compared with its
torch composition: the histogram equal, the crop within one ulp of 1 and the quantiser within one digital number (torch's own
division and fused arithmetic are not pinned; `bit_equal_to_torch` says whether they agreed), or the tool stops.
Usage: radiometry_bench.py [--iters 100] [--reps 5] [--scenes 96]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffusionremotesensing_amd import augment  # noqa: E402
from diffusionremotesensing_amd import radiometry as R  # noqa: E402

SCENE, WINDOW, BANDS, BATCH = 512, 256, 13, 16


def _window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _compare(entries, iters, reps):
    for fn in entries.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in entries}
    for _ in range(reps):
        for name, fn in entries.items():
            times[name].append(_window_ms(fn, iters))
    return times


def _cycle(values):
    state = {"at": -1}

    def nxt():
        state["at"] = (state["at"] + 1) % len(values)
        return values[state["at"]]
    return nxt


def _d4(w, code):
    if code & 4:
        w = w.transpose(-1, -2)
    if code & 1:
        w = w.flip(-1)
    if code & 2:
        w = w.flip(-2)
    return w


def _row(what, case, moved, times, iters):
    row = {"launch": what, "case": case, "MB": round(moved / 1e6, 2), "iters": iters}
    for k, v in times.items():
        row[f"{k}_us"] = {"min": round(1e3 * min(v), 2), "median": round(1e3 * statistics.median(v), 2), "max": round(1e3 * max(v), 2)}
    med = {k: statistics.median(v) for k, v in times.items()}
    row["kernel_GBps"] = round(moved / med["kernel"] / 1e6, 1)
    row["kernel_over_torch_time"] = round(med["kernel"] / med["torch"], 4)
    return row, med


def _dn(i16):
    """The digital numbers of an int16 view of uint16 data as fp32 (torch indexes and stacks int16; uint16 has few kernels)."""
    return (i16.to(torch.int32) & 0xFFFF).to(torch.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "radiometry_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    table = np.array([(100 + 10 * c, 9000 + 500 * c) for c in range(BANDS)], dtype=np.float32)
    td = R.device_table(table, dev)
    lo, span = td[:, 0].reshape(1, BANDS, 1, 1), (td[:, 1] - td[:, 0]).reshape(1, BANDS, 1, 1)
    nan = torch.tensor(float("nan"), device=dev)

    # ---- crop ---------------------------------------------------------------------------------------------------------
    i16 = torch.randint(-32768, 32768, (args.scenes, BANDS, SCENE, SCENE), generator=gen, dtype=torch.int16, device=dev)
    i16[:, :, :64, :64] = 0  # a no-data corner in every scene
    u16 = i16.view(torch.uint16)
    rng = np.random.default_rng(1)
    for name, codes in (("code0", [0]), ("transposing", [5]), ("mixed", list(range(8)))):
        host = []
        for k in range(32):
            items = augment.draw_items(rng, rng.permutation(args.scenes)[:BATCH], SCENE, SCENE, WINDOW, "none")
            items[:, 3] = [codes[(k + i) % len(codes)] for i in range(BATCH)]
            host.append(items)
        pairs = _cycle([(h, torch.from_numpy(h).to(dev)) for h in host])

        def torch_crop(items=None, marked=True):
            items = pairs()[0] if items is None else items
            w = torch.stack([_d4(i16[s, :, y:y + WINDOW, x:x + WINDOW], c) for s, y, x, c in items.tolist()])
            hr = ((_dn(w) - lo) / span).clamp(0.0, 1.0)
            return (hr, torch.where((w == 0).all(dim=1, keepdim=True), nan, hr)) if marked else (hr, None)
        got, want = R.crop_d4_u16_f32(u16, torch.from_numpy(host[0]).to(dev), WINDOW, td, nodata=0), torch_crop(host[0])
        assert torch.equal(torch.isnan(got[1]), torch.isnan(want[1])) and torch.allclose(got[0], want[0], rtol=0, atol=2.0 ** -23), name
        same = bool(torch.equal(got[0], want[0]) and torch.equal(got[1].nan_to_num(-1.0), want[1].nan_to_num(-1.0)))
        for marked in (False, True):
            times = _compare({"kernel": lambda: R.crop_d4_u16_f32(u16, pairs()[1], WINDOW, td, nodata=0 if marked else None),
                              "torch": lambda: torch_crop(marked=marked)}, args.iters, args.reps)
            moved = BATCH * BANDS * WINDOW * WINDOW * (2 + 4 + (4 if marked else 0))
            row, med = _row("crop_d4_u16_f32", f"{name}{', marked' if marked else ''}", moved, times, args.iters)
            print(json.dumps({**row, "bit_equal_to_torch": same}), flush=True)
    # the 8-bit sibling on a uint8 cache of the same shape, the same items, in the same session
    u8 = torch.randint(0, 256, (args.scenes, BANDS, SCENE, SCENE), generator=gen, dtype=torch.uint8, device=dev)
    labels = torch.arange(args.scenes, dtype=torch.int64, device=dev)
    times = _compare({"kernel": lambda: R.crop_d4_u16_f32(u16, pairs()[1], WINDOW, td),
                      "u8": lambda: augment.crop_d4_u8_f32(u8, labels, pairs()[1], WINDOW)}, args.iters, args.reps)
    m16, m8 = statistics.median(times["kernel"]), statistics.median(times["u8"])
    b16, b8 = BATCH * BANDS * WINDOW * WINDOW * 6, BATCH * BANDS * WINDOW * WINDOW * 5
    print(json.dumps({"launch": "crop_d4_u16_f32 vs crop_d4_u8_f32", "case": "mixed", "u16_us": round(1e3 * m16, 2), "u8_us": round(1e3 * m8, 2),
                      "u16_GBps": round(b16 / m16 / 1e6, 1), "u8_GBps": round(b8 / m8 / 1e6, 1)}), flush=True)
    del u8, i16, u16

    # ---- histogram ----------------------------------------------------------------------------------------------------
    shape = (16, BANDS, SCENE, SCENE)
    uniform = torch.randint(-32768, 32768, shape, generator=gen, dtype=torch.int16, device=dev)
    scene = torch.from_numpy(np.minimum(np.random.default_rng(2).gamma(2.0, 150.0, shape), 65535).astype(np.uint16).view(np.int16)).to(dev)
    constant = torch.full(shape, 4242, dtype=torch.int16, device=dev)
    for name, cache in (("uniform", uniform), ("scene-like", scene), ("constant planes", constant)):
        def torch_hist(cache=cache):
            v = cache.to(torch.int64) & 0xFFFF
            return torch.stack([torch.bincount(v[:, c].reshape(-1), minlength=65536) for c in range(BANDS)])
        assert torch.equal(R.hist_u16(cache.view(torch.uint16)), torch_hist()), name
        times = _compare({"kernel": lambda cache=cache: R.hist_u16(cache.view(torch.uint16)), "torch": torch_hist},
                         max(args.iters // 10, 3), args.reps)
        row, _ = _row("hist_u16", name, cache.numel() * 2, times, max(args.iters // 10, 3))
        print(json.dumps(row), flush=True)
    del uniform, scene, constant

    # ---- quantize -----------------------------------------------------------------------------------------------------
    x = torch.rand((BATCH, BANDS, WINDOW, WINDOW), generator=gen, device=dev) * 1.2 - 0.1
    x.view(-1)[::1001] = float("nan")

    def torch_quantize():
        v = (x.clamp(0.0, 1.0) * span + lo).round().clamp(0.0, 65535.0)
        return torch.where(torch.isnan(x), 7.0, v).to(torch.int32).to(torch.int16)  # (the low 16 bits: the uint16 value)
    got, want = R.quantize_u16(x, td, fill=7).view(torch.int16), torch_quantize()
    assert int(((got.to(torch.int32) & 0xFFFF) - (want.to(torch.int32) & 0xFFFF)).abs().max()) <= 1
    times = _compare({"kernel": lambda: R.quantize_u16(x, td, fill=7), "torch": torch_quantize}, args.iters, args.reps)
    row, _ = _row("quantize_u16", "16 x 13 x 256 x 256", x.numel() * 6, times, args.iters)
    print(json.dumps({**row, "bit_equal_to_torch": bool(torch.equal(got, want))}), flush=True)


if __name__ == "__main__":
    main()
