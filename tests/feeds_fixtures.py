"""Dataset folders the feed tests build under tmp_path, and the golden SAR -> NDVI folder (tools/make_golden_feeds.py)."""
import os

import numpy as np
import torch

GOLDEN_FEEDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feeds")


def golden_items():
    """The reference dataset's three (sar, ndvi) items of the golden folder, in its (sorted) order, and the file stems."""
    g = np.load(os.path.join(GOLDEN_FEEDS, "sar_items.npz"))
    return [(torch.from_numpy(g[f"sar_{i}"]), torch.from_numpy(g[f"ndvi_{i}"])) for i in range(3)], [str(n) for n in g["names"]]


def write_sar_folder(root, names, size, sar_channels=2, ndvi_channels=1, seed=0):
    """`root/{sar,opt}/<name>.pt` for every name: seeded images in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    for sub, c in (("sar", sar_channels), ("opt", ndvi_channels)):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
        for name in names:
            torch.save(torch.rand((c, size, size), generator=gen) * 2 - 1, os.path.join(root, sub, name + ".pt"))


def write_class_tree(root, size=8):
    """Classes b_cls, a_cls, c_cls (created in this order) holding, with Pillow: a nested sub-folder, a notes.txt that is no
    sample, an upper-case .PNG, a grey-scale PNG and a 5 x 7 image that the loader has to resize.  Returns the samples in the
    order ImageFolder lists them: (path relative to root, label)."""
    from PIL import Image
    rng = np.random.default_rng(5)

    def rgb(path, w=size, h=size):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)

    rgb(os.path.join(root, "b_cls", "z.png"))
    rgb(os.path.join(root, "b_cls", "B.PNG"))
    rgb(os.path.join(root, "a_cls", "sub", "n.png"))
    rgb(os.path.join(root, "a_cls", "m.png"), w=5, h=7)
    with open(os.path.join(root, "a_cls", "notes.txt"), "w") as f:
        f.write("not an image\n")
    os.makedirs(os.path.join(root, "c_cls"))
    Image.fromarray(rng.integers(0, 256, (size, size), dtype=np.uint8)).save(os.path.join(root, "c_cls", "grey.png"))
    # a_cls: its own files before those of a_cls/sub; b_cls: 'B.PNG' < 'z.png'
    return [("a_cls/m.png", 0), ("a_cls/sub/n.png", 0), ("b_cls/B.PNG", 1), ("b_cls/z.png", 1), ("c_cls/grey.png", 2)]


def pillow_bytes(path, size):
    """(3, S, S) uint8: the Pillow calls of ImageFolder's loader followed by transforms.Resize((S, S)) on a PIL image."""
    from PIL import Image
    y = Image.open(path).convert("RGB")
    if y.size != (size, size):
        y = y.resize((size, size), Image.BILINEAR)
    return torch.from_numpy(np.moveaxis(np.asarray(y, dtype=np.uint8), -1, 0).copy())
