"""On-device data feeds of the SAR -> NDVI and the generation trainers: the pattern of `degradation.py` for
the two sibling datasets.  The dataset folder is decoded ONCE on the host (`load_sar_ndvi_folder`, `load_class_folder_u8`), kept
as a cache on the device, and every batch is one HIP launch (`drs_gather_pairs_f32`, `drs_gather_u8_f32`, csrc/feed.hip): no
per-item host work and no host-to-device copy per step.

Kept from the reference: `get_data_SAR_TO_NDVI` (utils.py:40-91) - the files of `<root>/sar` in `sorted(os.listdir(...))` order,
each paired with the file of the same name in `<root>/opt`, `data_format` 'torch' / 'numpy', no transform, `(img + 1) / 2` - and
torchvision's `ImageFolder` + `Resize((S, S))` + `ToTensor` of the generation launch (generate_new_imgs/
train_diffusion_generation.py:574-584), restated here because torchvision is not a dependency: classes = the sorted
sub-directories, samples class by class in a sorted recursive walk, `Image.open(p).convert("RGB")`, Pillow's BILINEAR resize, bytes
/ 255.  Changed: the cache on the device; with several ranks every rank reads its own equal shard (every world-th sample, the
remainder left out) where DistributedSampler pads with repeats; the batch order is `torch.randperm(L)` per epoch as in a shuffling
DataLoader, but drawn from the feed's own `generator` argument.  Not covered: `data_format='PIL'` of the SAR dataset.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from .degradation import MAX_BANDS, load_npy_u8

# torchvision.datasets.folder.IMG_EXTENSIONS
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def _shard(items, what, rank, world_size, limit):
    """This rank's part of a sample list, as `degradation.load_image_folder_u8` cuts it: the first `limit` items of the whole
    list, or every world-th item with equal shard sizes (the ranks must run the same number of steps per epoch), the remainder
    left out and counted on rank 0."""
    if limit is not None:
        return items[:limit]
    per_rank = len(items) // world_size
    if per_rank == 0:
        raise ValueError(f"dataset of {len(items)} samples in {what} cannot be sharded over {world_size} ranks")
    if len(items) % world_size and rank == 0:
        print(f"{what}: {len(items) % world_size} of {len(items)} samples left out (equal shards over {world_size} ranks)")
    return items[rank::world_size][:per_rank]


def _check_cache(name, t, dtype, on_device=True):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 4 or t.shape[0] < 1:
        raise RuntimeError(f"{name} must be a non-empty (L, C, H, W) {dtype} tensor")
    if on_device and not t.is_cuda:
        raise RuntimeError(f"{name} must be on a ROCm device (no CPU fallback)")
    return t.contiguous()


def _check_idx(idx, device):
    if not isinstance(idx, torch.Tensor) or idx.device != device or idx.dtype != torch.int64 or idx.dim() != 1:
        raise RuntimeError("idx must be a 1-D int64 tensor on the cache's device")
    return idx.contiguous()


def gather_pairs(sar, ndvi, idx):
    """(sar[idx] + 1) / 2, (ndvi[idx] + 1) / 2 for two (L, C, H, W) fp32 caches and an int64 index vector, all on one ROCm
    device, in one launch (drs_gather_pairs_f32).  A row whose index is outside [0, L) comes back as zeros."""
    lib = _lib.load()
    sar, ndvi = _check_cache("sar", sar, torch.float32), _check_cache("ndvi", ndvi, torch.float32)
    if ndvi.device != sar.device or ndvi.shape[0] != sar.shape[0]:
        raise RuntimeError(f"gather_pairs: caches of {sar.shape[0]} and {ndvi.shape[0]} items on {sar.device} / {ndvi.device}")
    idx = _check_idx(idx, sar.device)
    n = idx.shape[0]
    sar_out = torch.empty((n,) + tuple(sar.shape[1:]), dtype=torch.float32, device=sar.device)
    ndvi_out = torch.empty((n,) + tuple(ndvi.shape[1:]), dtype=torch.float32, device=sar.device)
    if n == 0:
        return sar_out, ndvi_out
    with torch.cuda.device(sar.device):
        st = lib.drs_gather_pairs_f32(C.c_void_p(sar.data_ptr()), C.c_void_p(ndvi.data_ptr()), C.c_void_p(idx.data_ptr()), n,
                                      sar.shape[0], sar[0].numel(), ndvi[0].numel(), C.c_void_p(sar_out.data_ptr()),
                                      C.c_void_p(ndvi_out.data_ptr()),
                                      C.c_void_p(torch.cuda.current_stream(sar.device).cuda_stream))
    _lib.check(st, "drs_gather_pairs_f32")
    return sar_out, ndvi_out


def gather_u8(u8, labels, idx):
    """u8[idx].float() / 255, labels[idx] for a (L, C, H, W) uint8 cache, its (L,) int64 labels and an int64 index vector, all on
    one ROCm device, in one launch (drs_gather_u8_f32).  A row whose index is outside [0, L) comes back as zeros with label -1."""
    lib = _lib.load()
    u8 = _check_cache("u8", u8, torch.uint8)
    if not isinstance(labels, torch.Tensor) or labels.device != u8.device or labels.dtype != torch.int64 or \
            tuple(labels.shape) != (u8.shape[0],):
        raise RuntimeError(f"gather_u8: labels must be {u8.shape[0]} int64 values on the cache's device")
    labels, idx = labels.contiguous(), _check_idx(idx, u8.device)
    n = idx.shape[0]
    img = torch.empty((n,) + tuple(u8.shape[1:]), dtype=torch.float32, device=u8.device)
    lab = torch.empty((n,), dtype=torch.int64, device=u8.device)
    if n == 0:
        return img, lab
    with torch.cuda.device(u8.device):
        st = lib.drs_gather_u8_f32(C.c_void_p(u8.data_ptr()), C.c_void_p(labels.data_ptr()), C.c_void_p(idx.data_ptr()), n,
                                   u8.shape[0], u8[0].numel(), C.c_void_p(img.data_ptr()), C.c_void_p(lab.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream(u8.device).cuda_stream))
    _lib.check(st, "drs_gather_u8_f32")
    return img, lab


def nodata_pixels(img, nodata):
    """(..., 1, H, W) bool: the no-data pixels of fp32 images (..., C, H, W) under the package's rule - any band NaN or, when
    `nodata` is a number, all bands equal to it as fp32 ("nan" / True: the NaN rule alone)."""
    out = torch.isnan(img).any(dim=-3, keepdim=True)
    if nodata is True or (isinstance(nodata, str) and nodata.lower() == "nan"):
        return out
    if nodata is None or isinstance(nodata, (str, bool)):
        raise ValueError(f"nodata={nodata!r} must be 'nan', True or a number")
    value = torch.tensor(float(nodata), dtype=torch.float32)
    if torch.isinf(value):
        raise ValueError("nodata must be finite or NaN")
    return out if torch.isnan(value) else out | (img == value).all(dim=-3, keepdim=True)


def load_sar_ndvi_folder(root_dir, data_format="torch", rank=0, world_size=1, limit=None, nodata=None):
    """Read side of the reference's `get_data_SAR_TO_NDVI(root_dir, data_format=...)` (utils.py:54-85): the files of
    `root_dir/sar` in `sorted(os.listdir(...))` order, each with the file of the same name in `root_dir/opt`, as two fp32 host
    tensors (sar (L, Cs, H, W), ndvi (L, Cn, H, W)) holding the values of the files - the `(img + 1) / 2` of the dataset item
    happens per batch on the device (DeviceSarNdviFeed).  'torch': `.pt` files holding one tensor each; 'numpy': `.npy` files,
    `torch.tensor(np.load(p)).to(torch.float)`.  `rank` / `world_size` / `limit` as in `degradation.load_image_folder_u8`.
    `nodata` ("nan" or the files' no-data value; None: the files as they are) marks no-data pixels in band, once, here on the
    host: a no-data NDVI pixel (`nodata_pixels`) becomes NaN in all NDVI bands, and a no-data SAR pixel gets its SAR bands set
    to 0.0 - the network is never fed a NaN - and its NDVI bands set to NaN.  The gathers and crops carry a NaN untouched, so a
    `Diffusion` with `nodata = True` finds the mask in every batch."""
    if data_format not in ("torch", "numpy"):
        raise ValueError(f"data_format must be 'torch' or 'numpy', got {data_format!r}")
    sar_dir, opt_dir = os.path.join(root_dir, "sar"), os.path.join(root_dir, "opt")
    names = _shard(sorted(os.listdir(sar_dir)), root_dir, rank, world_size, limit)

    def read(path):
        if data_format == "numpy":
            img = torch.tensor(np.load(path, allow_pickle=False)).to(torch.float)
        else:
            img = torch.load(path, weights_only=True)
            if not isinstance(img, torch.Tensor):
                raise ValueError(f"{path}: expected one tensor, got {type(img).__name__}")
            img = img.to(torch.float)
        if img.dim() != 3:
            raise ValueError(f"{path}: expected one (C, H, W) image, got shape {tuple(img.shape)}")
        if img.shape[0] > MAX_BANDS:
            raise ValueError(f"{path}: {img.shape[0]} bands, the networks take at most {MAX_BANDS}")
        return img

    sar, ndvi = [], []
    for name in names:
        if not os.path.isfile(os.path.join(opt_dir, name)):
            raise ValueError(f"{os.path.join(sar_dir, name)}: no partner {os.path.join(opt_dir, name)}")
        for images, path in ((sar, os.path.join(sar_dir, name)), (ndvi, os.path.join(opt_dir, name))):
            img = read(path)
            if images and img.shape != images[0].shape:
                raise ValueError(f"{path}: shape {tuple(img.shape)} differs from the {tuple(images[0].shape)} of the files before it")
            images.append(img)
    sar, ndvi = torch.stack(sar).contiguous(), torch.stack(ndvi).contiguous()
    if nodata is not None:
        no_sar = nodata_pixels(sar, nodata)
        no_ndvi = nodata_pixels(ndvi, nodata) | no_sar
        sar = torch.where(no_sar, torch.zeros((), dtype=sar.dtype), sar)
        ndvi = torch.where(no_ndvi, torch.full((), float("nan"), dtype=ndvi.dtype), ndvi)
    return sar, ndvi


def _epoch_order(length, shuffle, generator, device):
    order = torch.randperm(length, generator=generator) if shuffle else torch.arange(length)
    return order.to(device)


def _feed_augment(H, W, crop_size, augment, num_crops, augment_seed, augment_rank, fixed_crop):
    """The FeedAugment of a feed's crop / augmentation arguments, or None where they are the defaults: the feed then imports and
    calls nothing of augment.py."""
    if crop_size is None and augment == "none":
        return None
    from .augment import FeedAugment
    return FeedAugment(H, W, crop_size, augment, num_crops, augment_seed, augment_rank, fixed_crop)


class DeviceSarNdviFeed:
    """Iterable of (SAR, NDVI) fp32 batches in [0, 1] drawn from the two caches on the device: what
    `DataLoader(get_data_SAR_TO_NDVI(root), batch_size, shuffle)` yields.  `sar`, `ndvi`: (L, C, H, W) fp32 on the device, the
    values of the files (load_sar_ndvi_folder).

    `crop_size` / `augment` ("none", "flip", "d4") make the feed active (augment.py): every item is a
    crop_size window of its image (default: the whole, square image) under a symmetry of the mode, the same for both tensors of
    the pair, drawn from the feed's own `np.random.default_rng([augment_seed, augment_rank])`; an epoch is `num_crops` passes
    over the cache; `fixed_crop`: the centre window, no symmetry, one pass.  `last_items`: the last batch's (n, 4) host items."""

    def __init__(self, sar, ndvi, batch_size=16, shuffle=True, generator=None, crop_size=None, augment="none", num_crops=1,
                 augment_seed=0, augment_rank=0, fixed_crop=False):
        # (the device is checked where a batch is made: gather_pairs)
        self.sar, self.ndvi = _check_cache("sar", sar, torch.float32, False), _check_cache("ndvi", ndvi, torch.float32, False)
        if self.ndvi.shape[0] != self.sar.shape[0]:
            raise RuntimeError(f"{self.sar.shape[0]} SAR images for {self.ndvi.shape[0]} NDVI images")
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.generator = generator
        self._aug = _feed_augment(self.sar.shape[2], self.sar.shape[3], crop_size, augment, num_crops, augment_seed, augment_rank,
                                  fixed_crop)
        self.last_items = None

    def __len__(self):
        if self._aug is not None:
            return self._aug.num_batches(self.sar.shape[0], self.batch_size)
        return (self.sar.shape[0] + self.batch_size - 1) // self.batch_size

    def _crop(self, items):
        from .augment import crop_d4_pairs, upload_items
        return crop_d4_pairs(self.sar, self.ndvi, upload_items(items, self.sar.device), self._aug.size)

    def item(self, idx):
        """(SAR, NDVI) of one dataset item, (C, H, W) each: `dataset[idx]` of the reference's Dataset (an active feed: the centre
        window, no symmetry)."""
        if not 0 <= idx < self.sar.shape[0]:
            raise IndexError(f"item {idx} of a dataset of {self.sar.shape[0]}")
        if self._aug is not None:
            x, y = self._crop(self._aug.centre(idx))
            return x[0], y[0]
        x, y = gather_pairs(self.sar, self.ndvi, torch.tensor([idx], dtype=torch.int64).to(self.sar.device))
        return x[0], y[0]

    def epoch_order(self):
        """The index vector of one epoch of an active feed, on the host: `num_crops` orders drawn as one is drawn today."""
        n = self.sar.shape[0]
        return self._aug.epoch_order(lambda: _epoch_order(n, self.shuffle, self.generator, "cpu"))

    def __iter__(self):
        n = self.sar.shape[0]
        if self._aug is not None:
            order = self.epoch_order().numpy()
            for i in range(0, order.shape[0], self.batch_size):
                self.last_items = self._aug.items(order[i:i + self.batch_size])
                yield self._crop(self.last_items)
            return
        order = _epoch_order(n, self.shuffle, self.generator, self.sar.device)
        for i in range(0, n, self.batch_size):
            yield gather_pairs(self.sar, self.ndvi, order[i:i + self.batch_size])


def load_class_folder_u8(root_dir, image_size, rank=0, world_size=1):
    """Decode side of `datasets.ImageFolder(root_dir, transform=Compose([Resize((S, S)), ToTensor()]))` (reference
    generate_new_imgs/train_diffusion_generation.py:574-579), torchvision's rules restated: the classes are the sorted
    sub-directory names of `root_dir`, a sample's label is its class's index; samples come class by class, inside a class in a
    sorted recursive walk (`sorted(os.walk(dir, followlinks=True))`, file names sorted), only files whose lower-cased extension is
    in IMG_EXTENSIONS; a class without such a file raises FileNotFoundError.  Every image is `Image.open(p).convert("RGB")`,
    resized with Pillow's BILINEAR to (S, S) when its size differs (Resize on a PIL image), and kept as bytes: the `/ 255` of
    ToTensor happens per batch on the device (DeviceClassFeed).  Returns (u8 (L, C, S, S), labels (L,) int64, classes) on the host.

    Multispectral extension (this project's convention, degradation.load_npy_u8): `.npy` files in the class folders count as
    samples, one (H, W, C) float array in [0, 1] each; all samples of a dataset have the same band count.
    `rank` / `world_size`: only this rank's shard of the sample list is decoded (every world-th sample, equal shards); the
    classes are those of the whole folder on every rank."""
    from PIL import Image
    classes = sorted(e.name for e in os.scandir(root_dir) if e.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {root_dir}.")
    samples, empty = [], []
    for label, cls in enumerate(classes):
        before = len(samples)
        for folder, _, fnames in sorted(os.walk(os.path.join(root_dir, cls), followlinks=True)):
            samples += [(os.path.join(folder, f), label) for f in sorted(fnames) if f.lower().endswith(IMG_EXTENSIONS + (".npy",))]
        if len(samples) == before:
            empty.append(cls)
    if empty:
        raise FileNotFoundError(f"Found no valid file for the classes {', '.join(empty)}. Supported extensions are: "
                                f"{', '.join(IMG_EXTENSIONS + ('.npy',))}")
    samples = _shard(samples, root_dir, rank, world_size, None)
    planes = []
    for path, _ in samples:
        if path.lower().endswith(".npy"):
            planes.append(load_npy_u8(path, image_size))
            continue
        with Image.open(path) as f:
            y = f.convert("RGB")
        if y.size != (image_size, image_size):
            y = y.resize((image_size, image_size), Image.BILINEAR)
        planes.append(np.moveaxis(np.asarray(y, dtype=np.uint8), -1, 0))
    bands = sorted({p.shape[0] for p in planes})
    if len(bands) > 1:
        raise ValueError(f"samples of {root_dir} differ in band count {bands}")
    u8 = torch.from_numpy(np.ascontiguousarray(np.stack(planes)))
    return u8, torch.tensor([label for _, label in samples], dtype=torch.int64), classes


class _ClassItems:
    """`loader.dataset` of a DeviceClassFeed: what the reference's `train` and `launch` read from the ImageFolder -
    `dataset.classes` and `dataset[0][0].shape[0]`."""

    def __init__(self, feed):
        self._feed = feed
        self.classes = feed.classes

    def __len__(self):
        return self._feed.u8.shape[0]

    def __getitem__(self, idx):
        if not 0 <= idx < len(self):
            raise IndexError(f"item {idx} of a dataset of {len(self)}")
        if self._feed._aug is not None:  # an active feed: the centre window, no symmetry
            img, label = self._feed._crop(self._feed._aug.centre(idx))
            return img[0], int(label[0])
        img, label = gather_u8(self._feed.u8, self._feed.labels, torch.tensor([idx], dtype=torch.int64).to(self._feed.u8.device))
        return img[0], int(label[0])


class DeviceClassFeed:
    """Iterable of (img fp32 in [0, 1], label int64) device batches drawn from a uint8 cache on the device: what
    `DataLoader(ImageFolder(root, transform), batch_size, shuffle)` yields.  `u8`: (L, C, S, S) uint8, `labels`: (L,) int64, both
    on the device (load_class_folder_u8).  `crop_size`, `augment`, `num_crops`, `augment_seed`, `augment_rank`, `fixed_crop`,
    `last_items`: as in DeviceSarNdviFeed."""

    def __init__(self, u8, labels, classes, batch_size=16, shuffle=True, generator=None, crop_size=None, augment="none",
                 num_crops=1, augment_seed=0, augment_rank=0, fixed_crop=False):
        self.u8 = _check_cache("u8", u8, torch.uint8, False)  # (the device is checked where a batch is made: gather_u8)
        if not isinstance(labels, torch.Tensor) or labels.device != self.u8.device or labels.dtype != torch.int64 or \
                tuple(labels.shape) != (self.u8.shape[0],):
            raise RuntimeError(f"labels must be {self.u8.shape[0]} int64 values on the cache's device")
        self.labels = labels.contiguous()
        self.classes = list(classes)
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.generator = generator
        self._aug = _feed_augment(self.u8.shape[2], self.u8.shape[3], crop_size, augment, num_crops, augment_seed, augment_rank,
                                  fixed_crop)
        self.last_items = None
        self.dataset = _ClassItems(self)

    def __len__(self):
        if self._aug is not None:
            return self._aug.num_batches(self.u8.shape[0], self.batch_size)
        return (self.u8.shape[0] + self.batch_size - 1) // self.batch_size

    def _crop(self, items):
        from .augment import crop_d4_u8_f32, upload_items
        return crop_d4_u8_f32(self.u8, self.labels, upload_items(items, self.u8.device), self._aug.size)

    def epoch_order(self):
        """The index vector of one epoch of an active feed, on the host: `num_crops` orders drawn as one is drawn today."""
        n = self.u8.shape[0]
        return self._aug.epoch_order(lambda: _epoch_order(n, self.shuffle, self.generator, "cpu"))

    def __iter__(self):
        n = self.u8.shape[0]
        if self._aug is not None:
            order = self.epoch_order().numpy()
            for i in range(0, order.shape[0], self.batch_size):
                self.last_items = self._aug.items(order[i:i + self.batch_size])
                yield self._crop(self.last_items)
            return
        order = _epoch_order(n, self.shuffle, self.generator, self.u8.device)
        for i in range(0, n, self.batch_size):
            yield gather_u8(self.u8, self.labels, order[i:i + self.batch_size])
