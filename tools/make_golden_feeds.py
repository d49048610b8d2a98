#!/usr/bin/env python3
"""Fixtures of the SAR -> NDVI data feed: a seeded dataset folder of 3 pairs in both file formats and the items the reference's
own `get_data_SAR_TO_NDVI` (utils.py:40-91) makes of it.  Runs ONLY in the build container (needs /root/reference); `utils.py`
imports torchvision, cv2 and imageio at module level, absent here and replaced by empty modules.
    python tools/make_golden_feeds.py   ->  tests/golden/feeds/{pt,npy}/train/{sar,opt}/*, tests/golden/feeds/sar_items.npz
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
for name in ("torchvision", "torchvision.transforms", "torchvision.models", "torchvision.datasets", "cv2", "imageio"):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.path.insert(0, REF)
sys.dont_write_bytecode = True
import utils as ref_utils  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "feeds")
NAMES = ["s_10", "s_2", "a_7"]  # creation order; sorted: a_7, s_10, s_2
rng = np.random.default_rng(11)
for fmt in ("pt", "npy"):
    for sub in ("sar", "opt"):
        os.makedirs(os.path.join(OUT, fmt, "train", sub), exist_ok=True)
for k, name in enumerate(NAMES):
    sar = rng.uniform(-1.5, 1.5, (2, 8, 8)).astype(np.float32)
    ndvi = rng.uniform(-1.5, 1.5, (1, 8, 8)).astype(np.float32)
    sar[0, 0, :3] = ndvi[0, k, :3] = (-1.0, 0.0, 1.0)  # the ends and the middle of the range the reference assumes
    for sub, a in (("sar", sar), ("opt", ndvi)):
        torch.save(torch.from_numpy(a.copy()), os.path.join(OUT, "pt", "train", sub, name + ".pt"))
        np.save(os.path.join(OUT, "npy", "train", sub, name + ".npy"), a)

items = {}
for fmt, data_format in (("pt", "torch"), ("npy", "numpy")):
    ds = ref_utils.get_data_SAR_TO_NDVI(os.path.join(OUT, fmt, "train"), data_format=data_format)
    assert len(ds) == 3
    got = [ds[i] for i in range(3)]
    if items:  # both formats hold the same values: one set of expected items
        assert all(np.array_equal(items[f"sar_{i}"], got[i][0].numpy()) and np.array_equal(items[f"ndvi_{i}"], got[i][1].numpy())
                   for i in range(3))
    for i, (s, n) in enumerate(got):
        items[f"sar_{i}"], items[f"ndvi_{i}"] = s.numpy(), n.numpy()
items["names"] = np.array([os.path.splitext(n)[0] for n in ds.sar_ndvi_filenames])
np.savez_compressed(os.path.join(OUT, "sar_items.npz"), **items)
print("wrote", OUT, list(items["names"]))
