"""16-bit radiometry: a uint16 scene cache beside the uint8 one, band ranges, and the device feed that reads it (DESIGN.md
section 29; not in the reference, whose datasets are 8-bit).

Sentinel-2, Landsat and PlanetScope products are 12- to 16-bit digital numbers (DN) whose bands differ in range by an order of
magnitude and whose no-data value is 0.  Everything behind the cache is fp32, so the only place that loses their precision is
the cache itself: here it holds the DN as they are, (L, C, H, W) uint16, and a `DataRange` - a (C, 2) fp32 table (lo_c, hi_c),
hi_c > lo_c, both in 0 .. 65535 - says how a band becomes [0, 1]:

    normalise   x = min(max((float(v) - lo_c) / (hi_c - lo_c), 0), 1)
    quantise    v = clamp(rint(min(max(x, 0), 1) * (hi_c - lo_c) + lo_c), 0, 65535)      (rint to even; NaN -> fill)

in fp32, one correctly rounded operation per step, the span formed once; quantise(normalise(v)) == v on [lo_c, hi_c].
`normalise_host` / `quantize_host` are that definition in numpy; csrc/radiometry.hip has the three launches (`hist_u16`,
`crop_d4_u16_f32`, `quantize_u16` here).  A range is given (`LO,HI`, `LO,HI;LO,HI;...`) or taken from the training cache
(`auto[:PLO,PHI]`): per band the exact order statistics of 0-based rank floor(p / 100 (n_c - 1)) among its n_c counted
pixels, read off the histogram without interpolation (`range_from_counts`).

`DeviceU16SuperresFeed` is `degradation.DeviceSuperresFeed` for such a cache.  There is no 16-bit Pillow arithmetic to be
bit-exact with, so its degradation IS the un-rounded separable operator `consistency.SeparableOperator.downblur`, applied
with `hip_ops.sep_apply` and clamped: lr = clamp(A_y hr A_x^T, 0, 1), left un-quantised - the training degradation and the
LR-consistency operator are the same matrix.  A pixel whose C stored values all equal `nodata` is marked NaN in all bands of
the HR target (the marker of DESIGN.md section 27); the LR image is made from the stored values.

Not built: 16-bit SAR -> NDVI and generation feeds, scores in DN units, a 16-bit resize (files must have the cache's size),
DownBlurNoise / BSRGAN on this cache, a quantised LR image, GeoTIFF metadata."""
import argparse
import ctypes as C
import math
import os
import random

import numpy as np
import torch

from . import _lib
from .degradation import MAX_BANDS

U16_MAX = 65535
DEFAULT_RANGE = "0,65535"
DEFAULT_PERCENTILES = (0.5, 99.5)


# ---------------------------------------------------------------------------------------------
# band ranges (host)
# ---------------------------------------------------------------------------------------------
def check_table(table, bands=None):
    """`table` as a contiguous (C, 2) float32 array, ValueError unless 0 <= lo_c < hi_c <= 65535 in every row (and C == bands)."""
    t = np.ascontiguousarray(np.asarray(table.detach().cpu() if isinstance(table, torch.Tensor) else table, dtype=np.float32))
    if t.ndim != 2 or t.shape[1] != 2 or not 1 <= t.shape[0] <= MAX_BANDS:
        raise ValueError(f"a data range is a (C, 2) table (lo, hi) with 1 <= C <= {MAX_BANDS}, got shape {tuple(t.shape)}")
    if not (np.isfinite(t).all() and (t >= 0).all() and (t <= U16_MAX).all() and (t[:, 1] > t[:, 0]).all()):
        raise ValueError(f"a data range needs 0 <= LO < HI <= {U16_MAX} in every band, got {t.tolist()}")
    if bands is not None and t.shape[0] != bands:
        raise ValueError(f"the data range names {t.shape[0]} bands, the images have {bands}")
    return t


def range_table(pairs, bands):
    """The (bands, 2) float32 table of a list of (lo, hi): one pair stands for every band."""
    pairs = [tuple(p) for p in pairs]
    if len(pairs) == 1:
        pairs = pairs * int(bands)
    return check_table(pairs, bands)


def parse_data_range(text):
    """--data_range: ("fixed", [(lo, hi), ...]) for `LO,HI` (all bands) or `LO,HI;LO,HI;...` (one per band), ("auto", plo, phi)
    for `auto[:PLO,PHI]` (default auto:0.5,99.5).  ValueError for anything else."""
    text = str(text).strip()
    if text.lower().startswith("auto"):
        rest = text[4:]
        if not rest:
            return ("auto",) + DEFAULT_PERCENTILES
        try:
            if not rest.startswith(":"):
                raise ValueError
            plo, phi = (float(v) for v in rest[1:].split(","))
        except ValueError:
            raise ValueError(f"--data_range {text!r} must be auto or auto:PLO,PHI") from None
        if not 0.0 <= plo < phi <= 100.0:
            raise ValueError(f"--data_range {text!r} needs 0 <= PLO < PHI <= 100")
        return "auto", plo, phi
    try:
        pairs = []
        for part in text.split(";"):
            lo, hi = (float(v) for v in part.split(","))
            pairs.append((lo, hi))
    except ValueError:
        raise ValueError(f"--data_range {text!r} must be LO,HI or LO,HI;LO,HI;... or auto[:PLO,PHI]") from None
    check_table(pairs)
    return "fixed", pairs


def cli_data_range(text):
    """The value of --data_range, checked while the command line is parsed; kept as its text."""
    try:
        parse_data_range(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None
    return text


def format_table(table):
    return ";".join(f"{lo:g},{hi:g}" for lo, hi in check_table(table).tolist())


def _band_shape(ndim, band_axis):
    shape = [1] * ndim
    shape[band_axis] = -1
    return shape


def normalise_host(v, table, band_axis=0):
    """The definition in numpy: fp32 min(max((float(v) - lo) / (hi - lo), 0), 1), the bands of `v` along `band_axis`."""
    v = np.asarray(v)
    t = check_table(table, v.shape[band_axis])
    lo = t[:, 0].reshape(_band_shape(v.ndim, band_axis))
    span = (t[:, 1] - t[:, 0]).reshape(lo.shape)  # (float32 - float32: the span, formed once)
    return np.minimum(np.maximum((v.astype(np.float32) - lo) / span, np.float32(0)), np.float32(1))


def quantize_host(x, table, fill=0, band_axis=0):
    """The inverse in numpy: uint16 clamp(rint(min(max(x, 0), 1) * span + lo), 0, 65535), rint to even, NaN -> fill."""
    x = np.asarray(x, dtype=np.float32)
    t = check_table(table, x.shape[band_axis])
    lo = t[:, 0].reshape(_band_shape(x.ndim, band_axis))
    span = (t[:, 1] - t[:, 0]).reshape(lo.shape)
    nan = np.isnan(x)
    c = np.minimum(np.maximum(np.where(nan, np.float32(0), x), np.float32(0)), np.float32(1))
    v = np.clip(np.rint(c * span + lo), 0, U16_MAX).astype(np.uint16)
    return np.where(nan, np.uint16(_check_u16("fill", fill)), v)


def _check_u16(name, value):
    if isinstance(value, bool) or int(value) != value or not 0 <= int(value) <= U16_MAX:
        raise ValueError(f"{name}={value!r} must be an integer in 0 .. {U16_MAX}")
    return int(value)


def range_from_counts(counts, plo=DEFAULT_PERCENTILES[0], phi=DEFAULT_PERCENTILES[1]):
    """The (C, 2) float32 table of per-band percentiles from a (C, 65536) histogram: the value of 0-based rank
    floor(p / 100 (n_c - 1)) among the band's n_c counted pixels - an exact order statistic, no interpolation
    (np.quantile's method="lower").  ValueError for an empty band and for a band whose two percentiles coincide."""
    counts = np.asarray(counts.detach().cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    if counts.ndim != 2 or counts.shape[1] != U16_MAX + 1:
        raise ValueError(f"counts must be (C, {U16_MAX + 1}), got {tuple(counts.shape)}")
    if not 0.0 <= plo < phi <= 100.0:
        raise ValueError(f"percentiles {plo}, {phi} need 0 <= PLO < PHI <= 100")
    table = np.zeros((counts.shape[0], 2), dtype=np.float32)
    for c, row in enumerate(counts):
        n = int(row.sum())
        if n == 0:
            raise ValueError(f"band {c} has no counted pixel: no percentile to take a data range from")
        cum = np.cumsum(row)
        lo, hi = (int(np.searchsorted(cum, math.floor(p / 100 * (n - 1)), side="right")) for p in (plo, phi))
        if lo == hi:
            raise ValueError(f"band {c}: the {plo:g}th and {phi:g}th percentiles coincide at {lo}: give --data_range LO,HI")
        table[c] = lo, hi
    return check_table(table)


def reduce_counts(counts):
    """The histogram summed over the ranks of the process group (one all-reduce, in place), so that every rank takes the same
    percentiles; the counts themselves where no group of more than one rank is up."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(counts, op=dist.ReduceOp.SUM)
    return counts


# ---------------------------------------------------------------------------------------------
# launches (device)
# ---------------------------------------------------------------------------------------------
def _check_cache(cache):
    if not isinstance(cache, torch.Tensor) or cache.dtype != torch.uint16 or cache.dim() != 4 or cache.shape[0] < 1:
        raise RuntimeError("cache must be a non-empty (L, C, H, W) torch.uint16 tensor")
    if not cache.is_cuda:
        raise RuntimeError("cache must be on a ROCm device (no CPU fallback)")
    if not 1 <= cache.shape[1] <= MAX_BANDS:
        raise RuntimeError(f"cache has {cache.shape[1]} bands, at most {MAX_BANDS} are taken")
    return cache.contiguous()


def _check_range_tensor(table, bands, device):
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (bands, 2) or table.device != device:
        raise RuntimeError(f"data_range must be a ({bands}, 2) float32 tensor on {device} (radiometry.device_table)")
    return table.contiguous()


def _nodata_arg(nodata):
    return -1 if nodata is None else _check_u16("nodata", nodata)


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def device_table(table, device):
    """A checked band-range table as the (C, 2) fp32 device tensor the launches take."""
    return torch.from_numpy(check_table(table)).to(device)


def hist_u16(cache, nodata=None):
    """(C, 65536) int64 on the device: how many pixels of band c of a (L, C, H, W) uint16 cache hold each value, pixels whose
    bands all equal `nodata` left out - exact, the same in every run (drs_hist_u16)."""
    lib = _lib.load()
    cache = _check_cache(cache)
    L, c, H, W = cache.shape
    counts = torch.empty((c, U16_MAX + 1), dtype=torch.int64, device=cache.device)
    with torch.cuda.device(cache.device):
        st = lib.drs_hist_u16(C.c_void_p(cache.data_ptr()), L, c, H, W, _nodata_arg(nodata), C.c_void_p(counts.data_ptr()),
                              _stream(cache))
    _lib.check(st, "drs_hist_u16")
    return counts


def crop_d4_u16_f32(cache, items, size, data_range, nodata=None, marked=None):
    """(hr, hr_marked): the windows of `items` (augment.py: (n, 4) int32 (src, y0, x0, code) on the device) out of a (L, C, H, W)
    uint16 cache, normalised with the (C, 2) fp32 device table `data_range`: (n, C, size, size) fp32, and the same values with NaN
    in all bands of every pixel whose stored values all equal `nodata` (`marked` False, the default without `nodata`: None).  One
    launch (drs_crop_d4_u16_f32); an invalid item comes back as zeros in both."""
    from .augment import _check_items
    lib = _lib.load()
    cache = _check_cache(cache)
    L, c, H, W = cache.shape
    items, size = _check_items(items, cache.device, size, H, W)
    data_range = _check_range_tensor(data_range, c, cache.device)
    marked = (nodata is not None) if marked is None else bool(marked)
    n = items.shape[0]
    hr = torch.empty((n, c, size, size), dtype=torch.float32, device=cache.device)
    hr_marked = torch.empty((n, c, size, size), dtype=torch.float32, device=cache.device) if marked else None
    if n == 0:
        return hr, hr_marked
    with torch.cuda.device(cache.device):
        st = lib.drs_crop_d4_u16_f32(C.c_void_p(cache.data_ptr()), C.c_void_p(items.data_ptr()), n, L, c, H, W, size,
                                     C.c_void_p(data_range.data_ptr()), _nodata_arg(nodata), C.c_void_p(hr.data_ptr()),
                                     C.c_void_p(hr_marked.data_ptr()) if marked else None, _stream(cache))
    _lib.check(st, "drs_crop_d4_u16_f32")
    return hr, hr_marked


def quantize_u16(x, data_range, fill=0):
    """(n, C, H, W) uint16: the digital numbers of fp32 images in [0, 1] under the (C, 2) fp32 device table `data_range`, a NaN
    as `fill` (drs_quantize_u16)."""
    lib = _lib.load()
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError("quantize_u16: x must be a (n, C, H, W) float32 tensor without an empty extent")
    if not x.is_cuda:
        raise RuntimeError("quantize_u16: x must be on a ROCm device (no CPU fallback)")
    x = x.contiguous()
    n, c, H, W = x.shape
    data_range = _check_range_tensor(data_range, c, x.device)
    out = torch.empty((n, c, H, W), dtype=torch.uint16, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.drs_quantize_u16(C.c_void_p(x.data_ptr()), n, c, H * W, C.c_void_p(data_range.data_ptr()),
                                  _check_u16("fill", fill), C.c_void_p(out.data_ptr()), _stream(x))
    _lib.check(st, "drs_quantize_u16")
    return out


def auto_range(cache, plo=DEFAULT_PERCENTILES[0], phi=DEFAULT_PERCENTILES[1], nodata=None, all_ranks=False):
    """The percentile table of a cache on the device: one histogram launch, with `all_ranks` summed over the process group
    (`reduce_counts`), then `range_from_counts` on the host."""
    counts = hist_u16(cache, nodata)
    return range_from_counts(reduce_counts(counts) if all_ranks else counts, plo, phi)


def resolve_range(spec, cache, nodata=None, all_ranks=False):
    """The (C, 2) float32 table of a --data_range text (None: the default 0,65535) for a cache on the device."""
    kind, *rest = parse_data_range(DEFAULT_RANGE if spec is None else spec)
    if kind == "auto":
        return auto_range(cache, rest[0], rest[1], nodata, all_ranks)
    return range_table(rest[0], cache.shape[1])


# ---------------------------------------------------------------------------------------------
# the cache (host)
# ---------------------------------------------------------------------------------------------
def load_folder_u16(root, size, rank=0, world_size=1, limit=None):
    """The images of `root` in `sorted(os.listdir(...))` order as ONE (L, C, size, size) uint16 host tensor; sorting, sharding,
    `limit` and the equal-shard rule are `degradation.load_image_folder_u8`'s.  A file is a `.npy` array of dtype uint16, (H, W, C)
    or (H, W), C <= MAX_BANDS, or a single-band 16-bit PNG / TIFF that Pillow opens as mode I;16.  Nothing is resized: a file of
    another size raises, as do a float `.npy`, an 8-bit image and a folder whose files differ in band count - naming the file."""
    from PIL import Image, UnidentifiedImageError
    names = [n for n in sorted(os.listdir(root)) if os.path.isfile(os.path.join(root, n))]
    if limit is not None:
        names = names[:limit]
    else:
        per_rank = len(names) // world_size
        if per_rank == 0:
            raise ValueError(f"dataset of {len(names)} images in {root} cannot be sharded over {world_size} ranks")
        if len(names) % world_size and rank == 0:
            print(f"{root}: {len(names) % world_size} of {len(names)} images left out (equal shards over {world_size} ranks)")
        names = names[rank::world_size][:per_rank]
    planes = []
    for name in names:
        path = os.path.join(root, name)
        if name.endswith(".npy"):
            a = np.load(path, allow_pickle=False)
            if a.dtype != np.uint16:
                raise ValueError(f"{path}: expected a uint16 array of digital numbers, got {a.dtype} (a float array in [0, 1] is "
                                 "the 8-bit loader's: drop --bit_depth 16)")
            if a.ndim == 2:
                a = a[:, :, None]
            if a.ndim != 3 or not 1 <= a.shape[2] <= MAX_BANDS:
                raise ValueError(f"{path}: expected one (H, W, C) or (H, W) array with 1 <= C <= {MAX_BANDS} bands, got "
                                 f"{tuple(a.shape)}")
            a = np.moveaxis(a, -1, 0)
        else:
            try:
                img = Image.open(path)
            except (UnidentifiedImageError, OSError) as e:
                raise ValueError(f"{path}: not an image Pillow can read ({e}); the dataset folders must hold image files only") from e
            with img as y:
                y.load()
                if not y.mode.startswith("I;16"):
                    raise ValueError(f"{path}: image mode {y.mode!r} is not a single-band 16-bit image (I;16)")
                a = np.asarray(y).astype(np.uint16)[None]
        if a.shape[1:] != (size, size):
            raise ValueError(f"{path}: {a.shape[1]} x {a.shape[2]} pixels, the cache is {size} x {size}: there is no 16-bit "
                             "resize, the files must already have --scene_size / --image_size")
        if planes and a.shape[0] != planes[0].shape[0]:
            raise ValueError(f"{path}: {a.shape[0]} bands, the files before it have {planes[0].shape[0]}")
        planes.append(np.ascontiguousarray(a))
    return torch.from_numpy(np.ascontiguousarray(np.stack(planes)))


def synthetic_u16(hr, scale=10000):
    """Seeded test scenes: float HR patches in [0, 1] as round(hr * scale) digital numbers, (L, C, H, W) uint16 on the host."""
    dn = (hr.detach().cpu().to(torch.float64) * scale).round().clamp(0, U16_MAX).numpy().astype(np.uint16)
    return torch.from_numpy(np.ascontiguousarray(dn))


# ---------------------------------------------------------------------------------------------
# the feed
# ---------------------------------------------------------------------------------------------
class DeviceU16SuperresFeed:
    """Iterable of (lr, hr) fp32 batches drawn from a uint16 HR cache on the device, with the surface of
    `degradation.DeviceSuperresFeed` (`__len__`, `__iter__`, `item`, `epoch_order`, `last_items`, `blur_radius`).  `hr_u16`:
    (L, C, H, W) uint16 on the device; `data_range`: a (C, 2) table (default 0,65535); `nodata`: the stored value that marks a
    no-data pixel when all its bands hold it - the feed then yields the NaN-marked target (a `Diffusion` with `nodata = True`).
    Every batch is one crop launch - window and symmetry per item as augment.py draws them (`crop_size`, `augment`, `num_crops`,
    `augment_seed`, `augment_rank`, `fixed_crop`), or the item (idx, 0, 0, 0) at the cache's own, square size - and one
    `hip_ops.sep_apply` of the un-rounded DownBlur operator on `hr`, clamped to [0, 1]; the LR image is not quantised.
    `blur_radius="random"` is drawn once per feed."""

    def __init__(self, hr_u16, magnification_factor, blur_radius=0.5, batch_size=16, shuffle=True, data_range=None, nodata=None,
                 crop_size=None, augment="none", num_crops=1, augment_seed=0, augment_rank=0, fixed_crop=False, generator=None):
        from .augment import FeedAugment
        from .consistency import SeparableOperator
        if not isinstance(hr_u16, torch.Tensor) or hr_u16.dtype != torch.uint16 or hr_u16.dim() != 4 or hr_u16.shape[0] < 1:
            raise RuntimeError("hr_u16 must be a non-empty (L, C, H, W) torch.uint16 tensor")
        self.hr = hr_u16.contiguous()
        L, c, H, W = self.hr.shape
        self._aug = None
        if crop_size is not None or augment != "none":
            self._aug = FeedAugment(H, W, crop_size, augment, num_crops, augment_seed, augment_rank, fixed_crop)
        elif H != W:
            raise ValueError(f"the 16-bit feed takes square windows: give crop_size for scenes of {H} x {W}")
        self.size = self._aug.size if self._aug is not None else H
        self.last_items = None
        self.magnification_factor = int(magnification_factor)
        if self.magnification_factor < 1 or self.size // self.magnification_factor < 1:
            raise ValueError(f"windows of {self.size} are too small for magnification {magnification_factor}")
        if blur_radius == "random":  # drawn once per dataset object, like the 8-bit feed
            blur_radius = random.triangular(0.5, 1.5, 1)
        self.blur_radius = float(blur_radius)
        self.batch_size, self.shuffle, self.generator = batch_size, shuffle, generator
        self.data_range = check_table(parse_data_range(DEFAULT_RANGE)[1] * c if data_range is None else data_range, c)
        self.nodata = None if nodata is None else _check_u16("nodata", nodata)
        self.operator = SeparableOperator.downblur((self.size, self.size), self.magnification_factor, self.blur_radius)
        self._table = None

    def __len__(self):
        passes = self._aug.passes if self._aug is not None else 1
        return (passes * self.hr.shape[0] + self.batch_size - 1) // self.batch_size

    def _plain_items(self, src):
        src = np.asarray(src).reshape(-1)
        out = np.zeros((src.shape[0], 4), dtype=np.int32)
        out[:, 0] = src
        return out

    def batch(self, items):
        """(lr, hr or the marked hr) of the (n, 4) host items."""
        from . import hip_ops
        from .augment import upload_items
        if self._table is None or self._table.device != self.hr.device:
            self._table = device_table(self.data_range, self.hr.device)
        hr, marked = crop_d4_u16_f32(self.hr, upload_items(items, self.hr.device), self.size, self._table, self.nodata)
        lr = hip_ops.sep_apply(hr, *self.operator.matrices(self.hr.device)).clamp_(0.0, 1.0)
        return lr, (marked if self.nodata is not None else hr)

    def item(self, idx):
        """(lr, hr) of one dataset item, (C, h, w) / (C, S, S): the centre window (an active feed) or the whole image, no symmetry."""
        if not 0 <= idx < self.hr.shape[0]:
            raise IndexError(f"item {idx} of a dataset of {self.hr.shape[0]}")
        x, y = self.batch(self._aug.centre(idx) if self._aug is not None else self._plain_items([idx]))
        return x[0], y[0]

    def epoch_order(self):
        """The index vector of one epoch, on the host: `num_crops` orders, each drawn as one pass is."""
        n = self.hr.shape[0]

        def one_pass():
            return torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        return self._aug.epoch_order(one_pass) if self._aug is not None else one_pass()

    def __iter__(self):
        order = self.epoch_order().numpy()
        for i in range(0, order.shape[0], self.batch_size):
            src = order[i:i + self.batch_size]
            self.last_items = self._aug.items(src) if self._aug is not None else self._plain_items(src)
            yield self.batch(self.last_items)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def add_radiometry_args(p, in_help=True):
    """--bit_depth / --data_range of the super-resolution trainer (`in_help` False: registered without a --help entry, like
    --prediction, because that help text is recorded) and of `evaluate`."""
    p.add_argument("--bit_depth", type=int, choices=(8, 16), default=8,
                   help="16: the dataset holds 16-bit digital numbers (uint16 .npy files, I;16 PNG / TIFF, or synthetic_u16[:N]) "
                        "kept in a uint16 cache and normalised with --data_range; DownBlur only, files at --scene_size / "
                        "--image_size; default 8" if in_help else argparse.SUPPRESS)
    p.add_argument("--data_range", type=cli_data_range, default=None,
                   help="with --bit_depth 16: LO,HI (all bands), LO,HI;LO,HI;... (one per band) or auto[:PLO,PHI] (per-band "
                        "percentiles of the training cache, default auto:0.5,99.5); default 0,65535 for training, the "
                        "snapshot's table otherwise" if in_help else argparse.SUPPRESS)
    return p


def is_u16(args):
    return int(getattr(args, "bit_depth", 8) or 8) == 16


def check_args(args):
    """ValueError for a command line that mixes the 8-bit and the 16-bit entrance, or asks the 16-bit one for what it has not."""
    spec = str(getattr(args, "dataset_path", None) or "")
    if not is_u16(args):
        if getattr(args, "data_range", None) is not None:
            raise ValueError("--data_range belongs to --bit_depth 16")
        if spec.startswith("synthetic_u16"):
            raise ValueError("--dataset_path synthetic_u16 needs --bit_depth 16")
        return args
    kind = str(getattr(args, "Degradation_type", "DownBlur")).lower()
    if kind == "downblurnoise":
        raise ValueError("--bit_depth 16 cannot be combined with --Degradation_type DownBlurNoise: its noise levels are defined "
                         "on bytes")
    if kind == "bsrgan":
        raise ValueError("--bit_depth 16 cannot be combined with --Degradation_type BSRGAN: the blind degradation is defined on "
                         "8-bit images")
    if kind not in ("downblur", "mtf"):
        raise ValueError("--bit_depth 16 needs --Degradation_type DownBlur or MTF")
    if spec.startswith("synthetic") and not spec.startswith("synthetic_u16"):
        raise ValueError(f"--bit_depth 16 reads a folder of 16-bit files or synthetic_u16[:N], not {spec!r}")
    return args
