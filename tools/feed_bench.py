#!/usr/bin/env python3
"""The two batch-gather kernels of the data feeds (csrc/feed.hip) next to the torch composition each replaces, in one process:
  SAR -> NDVI   B = 32, 2 + 1 bands, 128 x 128 (BASELINE config 4):  drs_gather_pairs_f32  vs  (cache[idx] + 1) / 2 twice
  generation    B = 64, 3 x 64 x 64 (BASELINE config 5):             drs_gather_u8_f32     vs  cache[idx].float().div(255), labels[idx]
and, for the rate of the kernels when a launch has enough rows to fill the chip, the same at 16 times the batch.
The caches are larger than the Infinity Cache (--sar_items / --class_items rows: 805 MB / 332 MB by default) and every call takes the next batch of a
seeded permutation, so the rows come from HBM.  HIP events around --iters calls after a warm-up; --reps windows per entry, the two
entries of a pair alternating; one JSON line per shape with min / median / max of the window means, the achieved GB/s against the
bytes a batch must move (rows read + rows written) and its share of the 6.29 TB/s a float4 copy reaches on this part.
Usage: feed_bench.py [--iters 1000] [--reps 5] [--sar_items 4096] [--class_items 27000]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffusionremotesensing_amd import feeds  # noqa: E402

HBM_COPY_GBPS = 6290.0  # measured float4 copy rate of an MI355X (8.0 TB/s in the data sheet)


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
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in entries}
    for _ in range(reps):
        for name, fn in entries.items():
            times[name].append(_window_ms(fn, iters))
    return times


def _batches(length, batch, dev, seed):
    """A cycling source of index batches: consecutive slices of one seeded permutation of the dataset."""
    order = torch.randperm(length, generator=torch.Generator().manual_seed(seed)).to(dev)
    state = {"at": 0}

    def nxt():
        if state["at"] + batch > length:
            state["at"] = 0
        idx = order[state["at"]:state["at"] + batch]
        state["at"] += batch
        return idx
    return nxt


def _row(name, shape, moved, times, iters):
    row = {"feed": name, "batch_shape": shape, "batch_MB": round(moved / 1e6, 2), "iters": iters}
    for k, v in times.items():
        row[f"{k}_us"] = {"min": round(1e3 * min(v), 2), "median": round(1e3 * statistics.median(v), 2), "max": round(1e3 * max(v), 2)}
        gbps = moved / statistics.median(v) / 1e6
        row[f"{k}_GBps"] = round(gbps, 1)
        row[f"{k}_hbm_fraction"] = round(gbps / HBM_COPY_GBPS, 4)
    row["kernel_over_torch_time"] = round(statistics.median(times["kernel"]) / statistics.median(times["torch"]), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sar_items", type=int, default=4096)
    ap.add_argument("--class_items", type=int, default=27000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "feed_bench needs a ROCm device"
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)

    sar = (torch.rand((args.sar_items, 2, 128, 128), generator=gen) * 2 - 1).to(dev)
    ndvi = (torch.rand((args.sar_items, 1, 128, 128), generator=gen) * 2 - 1).to(dev)
    for batch in (32, 512):
        nxt = _batches(args.sar_items, batch, dev, 1)

        def torch_pairs():
            idx = nxt()
            return (sar[idx] + 1) / 2, (ndvi[idx] + 1) / 2
        times = _compare({"kernel": lambda: feeds.gather_pairs(sar, ndvi, nxt()), "torch": torch_pairs}, args.iters, args.reps)
        moved = 2 * 4 * batch * (sar[0].numel() + ndvi[0].numel())
        print(json.dumps(_row("sar_to_ndvi", [batch, "2+1", 128, 128], moved, times, args.iters)), flush=True)
    del sar, ndvi

    u8 = torch.randint(0, 256, (args.class_items, 3, 64, 64), generator=gen, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 10, (args.class_items,), generator=gen).to(dev)
    for batch in (64, 1024):
        nxt = _batches(args.class_items, batch, dev, 2)

        def torch_u8():
            idx = nxt()
            return u8[idx].float().div(255), labels[idx]
        times = _compare({"kernel": lambda: feeds.gather_u8(u8, labels, nxt()), "torch": torch_u8}, args.iters, args.reps)
        moved = batch * (u8[0].numel() * (1 + 4) + 2 * 8)
        print(json.dumps(_row("generation", [batch, 3, 64, 64], moved, times, args.iters)), flush=True)


if __name__ == "__main__":
    main()
