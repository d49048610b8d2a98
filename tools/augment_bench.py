#!/usr/bin/env python3
"""The crop / dihedral launch of the device feeds (csrc/augment.hip) next to two yardsticks, in one process:
  class feed    B = 16 and 32, 3 bands, 512 x 512 uint8 scenes -> 256 x 256 fp32 windows:   drs_crop_d4_u8_f32
  SAR -> NDVI   B = 16 and 32, 2 + 1 bands, 512 x 512 fp32 scenes -> 256 x 256 windows:     drs_crop_d4_pairs_f32
each with all items on code 0 (a plain window), all on a transposing code (5: a quarter turn) and a mix of all eight codes,
random window offsets throughout, against
  torch    the composition the launch replaces: per item index, slice, flip / transpose, then stack and convert;
  gather   the plain drs_gather_u8_f32 / drs_gather_pairs_f32 launch that writes the same output bytes from a cache of 256 x 256
           images: what a transform-free copy reaches on the same device in the same run.
The scene caches are larger than the Infinity Cache (--scenes images: 805 MB of bytes / 1.6 GB of floats at 512) and every call
takes the next batch of seeded items, uploaded before the clock starts, so the windows come from HBM.  HIP events around --iters
calls after a warm-up; --reps windows per entry, the entries taking turns; one JSON line per (feed, batch, item set) with min /
median / max of the window means and the achieved GB/s against the bytes a batch must move (windows read + windows written).
Before timing, every item set's launch is compared with the torch composition at the timed size: equal, or the tool stops.
Usage: augment_bench.py [--iters 200] [--reps 5] [--scenes 1024] [--pair_scenes 512]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffusionremotesensing_amd import augment, feeds  # noqa: E402

SCENE, WINDOW = 512, 256
ITEM_SETS = {"code0": [0], "transposing": [5], "mixed": list(range(8))}


def _window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _compare(entries, iters, reps):
    """{name: [window mean in ms] * reps}; the entries take turns, window by window."""
    for fn in entries.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in entries}
    for _ in range(reps):
        for name, fn in entries.items():
            times[name].append(_window_ms(fn, iters))
    return times


def _item_batches(length, batch, codes, seed, count=64):
    """`count` seeded (batch, 4) int32 host item arrays: src from a permutation, random offsets, codes cycling through `codes`."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        src = rng.permutation(length)[:batch]
        items = augment.draw_items(rng, src, SCENE, SCENE, WINDOW, "none")
        items[:, 3] = [codes[(k + i) % len(codes)] for i in range(batch)]
        out.append(items)
    return out


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


def _torch_windows(cache, items):
    return torch.stack([_d4(cache[s, :, y:y + WINDOW, x:x + WINDOW], c) for s, y, x, c in items.tolist()])


def _row(feed, batch, item_set, moved, times, iters):
    row = {"feed": feed, "batch": batch, "items": item_set, "batch_MB": round(moved / 1e6, 2), "iters": iters}
    for k, v in times.items():
        row[f"{k}_us"] = {"min": round(1e3 * min(v), 2), "median": round(1e3 * statistics.median(v), 2), "max": round(1e3 * max(v), 2)}
        row[f"{k}_GBps"] = round(moved / statistics.median(v) / 1e6, 1)
    med = {k: statistics.median(v) for k, v in times.items()}
    row["kernel_over_torch_time"] = round(med["kernel"] / med["torch"], 3)
    row["kernel_over_gather_time"] = round(med["kernel"] / med["gather"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=1024)
    ap.add_argument("--pair_scenes", type=int, default=512)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    one = torch.tensor(255.0, device=dev)

    # ---- class feed: uint8 scenes -> fp32 windows ------------------------------------------------------------------------
    u8 = torch.randint(0, 256, (args.scenes, 3, SCENE, SCENE), generator=gen, dtype=torch.uint8, device=dev)
    labels = torch.arange(args.scenes, dtype=torch.int64, device=dev)
    small = torch.randint(0, 256, (4 * args.scenes, 3, WINDOW, WINDOW), generator=gen, dtype=torch.uint8, device=dev)
    small_labels = torch.arange(4 * args.scenes, dtype=torch.int64, device=dev)
    for batch in (16, 32):
        idx = _cycle([torch.randperm(4 * args.scenes, generator=torch.Generator().manual_seed(k))[:batch].to(dev) for k in range(64)])
        for name, codes in ITEM_SETS.items():
            host = _item_batches(args.scenes, batch, codes, 1)
            pairs = _cycle([(h, torch.from_numpy(h).to(dev)) for h in host])
            got = augment.crop_d4_u8_f32(u8, labels, torch.from_numpy(host[0]).to(dev), WINDOW)
            want = _torch_windows(u8, host[0]).float() / one
            assert torch.equal(got[0], want) and torch.equal(got[1], labels[torch.from_numpy(host[0][:, 0].astype(np.int64)).to(dev)])
            times = _compare({"kernel": lambda: augment.crop_d4_u8_f32(u8, labels, pairs()[1], WINDOW),
                              "gather": lambda: feeds.gather_u8(small, small_labels, idx()),
                              "torch": lambda: _torch_windows(u8, pairs()[0]).float().div(255)}, args.iters, args.reps)
            moved = batch * 3 * WINDOW * WINDOW * (1 + 4)
            print(json.dumps(_row("class_u8_f32", batch, name, moved, times, args.iters)), flush=True)
    del u8, small

    # ---- SAR -> NDVI: fp32 scene pairs -> fp32 window pairs -----------------------------------------------------------------
    n = args.pair_scenes
    sar = torch.rand((n, 2, SCENE, SCENE), generator=gen, device=dev) * 2 - 1
    ndvi = torch.rand((n, 1, SCENE, SCENE), generator=gen, device=dev) * 2 - 1
    sar_small = torch.rand((4 * n, 2, WINDOW, WINDOW), generator=gen, device=dev) * 2 - 1
    ndvi_small = torch.rand((4 * n, 1, WINDOW, WINDOW), generator=gen, device=dev) * 2 - 1
    for batch in (16, 32):
        idx = _cycle([torch.randperm(4 * n, generator=torch.Generator().manual_seed(k))[:batch].to(dev) for k in range(64)])
        for name, codes in ITEM_SETS.items():
            host = _item_batches(n, batch, codes, 2)
            pairs = _cycle([(h, torch.from_numpy(h).to(dev)) for h in host])

            def torch_pairs():
                items = pairs()[0]
                return (_torch_windows(sar, items) + 1) / 2, (_torch_windows(ndvi, items) + 1) / 2
            got = augment.crop_d4_pairs(sar, ndvi, torch.from_numpy(host[0]).to(dev), WINDOW)
            assert torch.equal(got[0], (_torch_windows(sar, host[0]) + 1) / 2) and torch.equal(got[1], (_torch_windows(ndvi, host[0]) + 1) / 2)
            times = _compare({"kernel": lambda: augment.crop_d4_pairs(sar, ndvi, pairs()[1], WINDOW),
                              "gather": lambda: feeds.gather_pairs(sar_small, ndvi_small, idx()),
                              "torch": torch_pairs}, args.iters, args.reps)
            moved = 2 * 4 * batch * 3 * WINDOW * WINDOW
            print(json.dumps(_row("sar_to_ndvi_pairs", batch, name, moved, times, args.iters)), flush=True)


if __name__ == "__main__":
    main()
