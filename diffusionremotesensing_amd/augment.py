"""Random crops and dihedral augmentation in front of the four device feeds.

A feed keeps its dataset decoded in a cache on the device and makes a batch from an index vector in one launch.  With
`crop_size` / `augment` set, that launch is one of csrc/augment.hip's instead: batch item i is described by four int32 values
`items[i] = (src, y0, x0, code)` - the S x S window of cache image `src` with top-left corner (y0, x0), transformed by the
dihedral code 0..7:

    if code & 4: w = w.swapaxes(-1, -2)     # transpose first
    if code & 1: w = w[..., ::-1]           # then reverse the columns
    if code & 2: w = w[..., ::-1, :]        # then reverse the rows

All bands of an item, and both tensors of a (SAR, NDVI) pair, get the same window and the same code.  What follows the launch
(DownBlur, the blind degradation, the trainers) is what it was: it sees a batch of S x S images.

Kept from the reference: its BSRGAN dataset's `num_crops` random patches per scene (utils.py:205-210, `random_crop` in
degradation_from_BSRGAN.py:584), as `num_crops` passes over the cache per epoch, every item a fresh window.  Not in the
reference: the eight symmetries, crops in the other three datasets, and that nothing is stored - windows are drawn per batch.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

AUGMENT_CODES = {"none": 1, "flip": 4, "d4": 8}  # how many of the codes 0..7 a mode draws from: flip = no transposition


# ---------------------------------------------------------------------------------------------
# items (host)
# ---------------------------------------------------------------------------------------------
def _check_window(H, W, size):
    if not 1 <= size <= min(H, W):
        raise ValueError(f"a window of {size} x {size} does not fit images of {H} x {W}")


def draw_items(rng, src, H, W, size, augment):
    """(n, 4) int32 host array (src, y0, x0, code) for the index vector `src`: the n codes, then the n row offsets, then the n
    column offsets, from the numpy Generator `rng` - uniform over the mode's codes and over every window that lies inside H x W."""
    if augment not in AUGMENT_CODES:
        raise ValueError(f"augment={augment!r} must be one of {tuple(AUGMENT_CODES)}")
    _check_window(H, W, size)
    src = np.asarray(src).reshape(-1)
    n = src.shape[0]
    code = rng.integers(0, AUGMENT_CODES[augment], n)
    y0 = rng.integers(0, H - size + 1, n)
    x0 = rng.integers(0, W - size + 1, n)
    return np.stack([src, y0, x0, code], axis=1).astype(np.int32)


def centre_items(src, H, W, size):
    """(n, 4) int32 host array of the fixed form: the centre window, code 0 (validation feeds, `item(idx)`)."""
    _check_window(H, W, size)
    src = np.asarray(src).reshape(-1)
    out = np.zeros((src.shape[0], 4), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2] = src, (H - size) // 2, (W - size) // 2
    return out


# ---------------------------------------------------------------------------------------------
# launches (device)
# ---------------------------------------------------------------------------------------------
def _check_cache(name, t, dtype):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 4 or t.shape[0] < 1:
        raise RuntimeError(f"{name} must be a non-empty (L, C, H, W) {dtype} tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be on a ROCm device (no CPU fallback)")
    return t.contiguous()


def _check_items(items, device, size, H, W):
    if not isinstance(items, torch.Tensor) or items.device != device or items.dtype != torch.int32 or items.dim() != 2 or \
            items.shape[1] != 4:
        raise RuntimeError("items must be a (n, 4) int32 tensor (src, y0, x0, code) on the cache's device")
    size = int(size)
    if not 1 <= size <= min(H, W):
        raise RuntimeError(f"a window of {size} x {size} does not fit images of {H} x {W}")
    return items.contiguous(), size


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def crop_d4_u8(cache, items, size):
    """The windows of `items` out of a (L, C, H, W) uint8 cache, as bytes: (n, C, size, size) uint8, one launch
    (drs_crop_d4_u8).  An invalid item (src, window or code out of range) comes back as zeros."""
    lib = _lib.load()
    cache = _check_cache("cache", cache, torch.uint8)
    L, c, H, W = cache.shape
    items, size = _check_items(items, cache.device, size, H, W)
    n = items.shape[0]
    out = torch.empty((n, c, size, size), dtype=torch.uint8, device=cache.device)
    if n == 0:
        return out
    with torch.cuda.device(cache.device):
        st = lib.drs_crop_d4_u8(C.c_void_p(cache.data_ptr()), C.c_void_p(items.data_ptr()), n, L, c, H, W, size,
                                C.c_void_p(out.data_ptr()), _stream(cache))
    _lib.check(st, "drs_crop_d4_u8")
    return out


def crop_d4_u8_f32(cache, labels, items, size):
    """(windows as float(b) / 255, labels[src]) for a (L, C, H, W) uint8 cache and its (L,) int64 labels: (n, C, size, size) fp32
    and (n,) int64, one launch (drs_crop_d4_u8_f32).  An invalid item comes back as zeros with label -1."""
    lib = _lib.load()
    cache = _check_cache("cache", cache, torch.uint8)
    L, c, H, W = cache.shape
    if not isinstance(labels, torch.Tensor) or labels.device != cache.device or labels.dtype != torch.int64 or \
            tuple(labels.shape) != (L,):
        raise RuntimeError(f"crop_d4_u8_f32: labels must be {L} int64 values on the cache's device")
    labels = labels.contiguous()
    items, size = _check_items(items, cache.device, size, H, W)
    n = items.shape[0]
    img = torch.empty((n, c, size, size), dtype=torch.float32, device=cache.device)
    lab = torch.empty((n,), dtype=torch.int64, device=cache.device)
    if n == 0:
        return img, lab
    with torch.cuda.device(cache.device):
        st = lib.drs_crop_d4_u8_f32(C.c_void_p(cache.data_ptr()), C.c_void_p(labels.data_ptr()), C.c_void_p(items.data_ptr()), n,
                                    L, c, H, W, size, C.c_void_p(img.data_ptr()), C.c_void_p(lab.data_ptr()), _stream(cache))
    _lib.check(st, "drs_crop_d4_u8_f32")
    return img, lab


def crop_d4_pairs(sar, ndvi, items, size):
    """The same windows of two fp32 caches (L, Cs, H, W) and (L, Cn, H, W) as (v + 1) / 2: (n, Cs, size, size) and (n, Cn, size,
    size) fp32, one launch (drs_crop_d4_pairs_f32).  An invalid item comes back as zeros in both."""
    lib = _lib.load()
    sar, ndvi = _check_cache("sar", sar, torch.float32), _check_cache("ndvi", ndvi, torch.float32)
    if ndvi.device != sar.device or ndvi.shape[0] != sar.shape[0] or ndvi.shape[2:] != sar.shape[2:]:
        raise RuntimeError(f"crop_d4_pairs: caches {tuple(sar.shape)} and {tuple(ndvi.shape)} on {sar.device} / {ndvi.device}")
    L, cs, H, W = sar.shape
    items, size = _check_items(items, sar.device, size, H, W)
    n = items.shape[0]
    sar_out = torch.empty((n, cs, size, size), dtype=torch.float32, device=sar.device)
    ndvi_out = torch.empty((n, ndvi.shape[1], size, size), dtype=torch.float32, device=sar.device)
    if n == 0:
        return sar_out, ndvi_out
    with torch.cuda.device(sar.device):
        st = lib.drs_crop_d4_pairs_f32(C.c_void_p(sar.data_ptr()), C.c_void_p(ndvi.data_ptr()), C.c_void_p(items.data_ptr()), n, L,
                                       cs, ndvi.shape[1], H, W, size, C.c_void_p(sar_out.data_ptr()),
                                       C.c_void_p(ndvi_out.data_ptr()), _stream(sar))
    _lib.check(st, "drs_crop_d4_pairs_f32")
    return sar_out, ndvi_out


# ---------------------------------------------------------------------------------------------
# what an active feed keeps
# ---------------------------------------------------------------------------------------------
class FeedAugment:
    """The crop / augmentation state of one device feed over a cache of H x W images: the window size, the mode, the passes per
    epoch and the feed's own item generator `np.random.default_rng([augment_seed, augment_rank])` - separate from the generator
    that orders the epoch and from everything the degradation draws.  `fixed_crop`: centre windows, code 0, one pass (validation)."""

    def __init__(self, H, W, crop_size=None, augment="none", num_crops=1, augment_seed=0, augment_rank=0, fixed_crop=False):
        if augment not in AUGMENT_CODES:
            raise ValueError(f"augment={augment!r} must be one of {tuple(AUGMENT_CODES)}")
        if crop_size is None:
            if H != W:
                raise ValueError(f"augment={augment!r} without crop_size takes the cache's own size, which must be square, not {H} x {W}")
            crop_size = H
        self.H, self.W, self.size = int(H), int(W), int(crop_size)
        _check_window(self.H, self.W, self.size)
        if int(num_crops) < 1:
            raise ValueError(f"num_crops={num_crops} must be >= 1")
        self.augment = augment
        self.fixed = bool(fixed_crop)
        self.passes = 1 if self.fixed else int(num_crops)
        self.rng = np.random.default_rng([int(augment_seed), int(augment_rank)])

    def num_batches(self, length, batch_size):
        return (self.passes * length + batch_size - 1) // batch_size

    def epoch_order(self, one_pass):
        """The index vector of an epoch: `passes` orders, each drawn by `one_pass()` as one pass is drawn today, concatenated."""
        return torch.cat([one_pass() for _ in range(self.passes)])

    def items(self, src):
        """The (n, 4) int32 host items of the batch whose index vector (host) is `src`."""
        if self.fixed:
            return centre_items(src, self.H, self.W, self.size)
        return draw_items(self.rng, src, self.H, self.W, self.size, self.augment)

    def centre(self, idx):
        return centre_items([idx], self.H, self.W, self.size)


def upload_items(items, device):
    """A batch's host items on the device (one 16 n byte upload)."""
    return torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32)).to(device)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def add_augment_args(p):
    """--scene_size / --augment / --augment_seed, and --num_crops where the parser does not have it already (the trainers'
    `main`, `evaluate.main`; not in the reference, whose --num_crops belongs to its BSRGAN dataset alone)."""
    p.add_argument("--scene_size", type=int, default=None,
                   help="keep the dataset as P x P scenes (P >= --image_size) and train on --image_size windows cut out of them "
                        "on the device; validation uses the centre windows.  Default: the dataset is kept at --image_size")
    p.add_argument("--augment", type=str, choices=tuple(AUGMENT_CODES), default="none",
                   help="per training item: none, flip (the four mirror images) or d4 (all eight symmetries of the square)")
    p.add_argument("--augment_seed", type=int, default=0, help="seed of the windows and symmetries (each rank draws its own)")
    text = ("passes over the dataset per epoch, every item a fresh random window / symmetry (the reference's BSRGAN dataset "
            "keeps num_crops frozen patches per scene); no effect unless --scene_size or --augment is given")
    for a in p._actions:
        if a.dest == "num_crops":
            a.help = text
            break
    else:
        p.add_argument("--num_crops", type=int, default=1, help=text)
    return p


def scene_size(args):
    """The cache's image size for a command line: --scene_size where given (>= --image_size, else ValueError), else --image_size."""
    scene = getattr(args, "scene_size", None)
    if scene is None:
        return args.image_size
    if scene < args.image_size:
        raise ValueError(f"--scene_size {scene} is smaller than --image_size {args.image_size}")
    return scene


def feed_kwargs(args, rank=0, fixed=False):
    """The crop / augmentation keyword arguments of a device feed for a command line; {} where neither --scene_size nor --augment is
    given (the feed is then exactly what it was).  `fixed`: a validation feed - centre windows, no augmentation."""
    scene, mode = getattr(args, "scene_size", None), getattr(args, "augment", "none")
    if scene is None and mode == "none":
        return {}
    crop = args.image_size if scene is not None else None
    if fixed:
        return {"crop_size": crop, "fixed_crop": True} if crop is not None else {}
    return {"crop_size": crop, "augment": mode, "num_crops": getattr(args, "num_crops", 1),
            "augment_seed": getattr(args, "augment_seed", 0), "augment_rank": rank}
