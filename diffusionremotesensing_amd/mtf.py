"""Sensor-MTF degradation (Wald's protocol; not in the reference): every band is blurred with the Gaussian
whose transfer function has the band's gain `g` at the LR Nyquist frequency, 1 / (2 m) cycles per HR pixel, and decimated by m.

Per axis: sigma = m sqrt(-2 ln g) / pi, L = ceil(3 sigma), n = 2 L + m taps; tap u of LR pixel i sits on HR index i m + u - L
(clamped into the image), weighs exp(-(u - L - (m - 1) / 2)^2 / (2 sigma^2)) - a window symmetric about the LR pixel's centre
(i + 0.5) m - 0.5, the convention of the network's bicubic up-sampling - normalised to sum 1 in float64 and rounded to fp32.  The
fp32 taps are THE operator: `hip_ops.fir_decimate` runs them as a FIR, `dense_axis` scatters the same numbers into the (h, H)
matrix of `consistency.SeparableOperator.mtf`, so the feed's degradation and the projection's operator are one map."""
import math
import numbers

import numpy as np
import torch

MIN_FACTOR, MAX_FACTOR = 2, 8      # m = 1 is refused: the sampled Gaussian aliases there (its discrete gain at Nyquist is 2 g)
MIN_NYQUIST, MAX_NYQUIST = 0.05, 0.6  # above 0.6 the sampled taps miss the gain by more than 2 % at m = 2
MAX_TAPS = 64                      # what drs_fir_decimate takes; the largest here is 46 (m = 8, g = 0.05)


def _check_factor(m, what="magnification_factor"):
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not MIN_FACTOR <= m <= MAX_FACTOR:
        raise ValueError(f"{what}={m!r} must be an integer in {MIN_FACTOR} .. {MAX_FACTOR} for an MTF degradation")
    return int(m)


def _check_gain(g, what="mtf_nyquist"):
    if isinstance(g, bool) or not isinstance(g, numbers.Real) or not MIN_NYQUIST <= g <= MAX_NYQUIST:
        raise ValueError(f"{what}={g!r} must be a number in {MIN_NYQUIST} .. {MAX_NYQUIST}")
    return float(g)


def nyquist_sigma(g, m):
    """The standard deviation, in HR pixels, of the Gaussian PSF whose MTF is `g` at 1 / (2 m) cycles per HR pixel."""
    g, m = _check_gain(g), _check_factor(m, "m")
    return m * math.sqrt(-2.0 * math.log(g)) / math.pi


def gaussian_taps(g, m):
    """(taps, L): the n = 2 L + m fp32 taps of one axis as a float64 array (each value an fp32 number), and the number of taps
    left of the LR pixel's first HR index."""
    sigma = nyquist_sigma(g, m)
    L = int(math.ceil(3.0 * sigma))
    u = np.arange(2 * L + m, dtype=np.float64)
    k = np.exp(-((u - L - (m - 1) / 2.0) ** 2) / (2.0 * sigma * sigma))
    k = k / k.sum()
    return k.astype(np.float32).astype(np.float64), L


def band_taps(gains, m):
    """(taps (n_ops, n) float64, L, band_op) for per-band gains: one row per DISTINCT gain, in order of first appearance, and for
    each band the row it uses.  Gains differ in L, so every row is centred in the widest window, n = 2 max(L) + m, with zeros
    around it: a zero tap leaves an fmaf chain's bits alone, so the padded row is the same FIR."""
    gains = [float(g) for g in gains]
    distinct = sorted(set(gains), key=gains.index)
    rows = [gaussian_taps(g, m) for g in distinct]
    left = max(L for _, L in rows)
    taps = np.stack([np.pad(k, (left - L, left - L)) for k, L in rows])
    return taps, left, [distinct.index(g) for g in gains]


def dense_axis(in_size, out_size, taps, left, m):
    """(out_size, in_size) float64: A[i, clamp(i m + u - left)] += taps[u] - the FIR with replicated edges as a matrix."""
    in_size, out_size, m = int(in_size), int(out_size), int(m)
    if out_size < 1 or out_size * m > in_size:
        raise ValueError(f"mtf: {out_size} LR pixels x {m} do not fit {in_size} HR pixels")
    A = np.zeros((out_size, in_size))
    for i in range(out_size):
        for u, k in enumerate(np.asarray(taps, dtype=np.float64)):
            A[i, min(max(i * m + u - int(left), 0), in_size - 1)] += k
    return A


def lr_shape(size_hw, m, lr_hw=None):
    """(h, w) of an (H, W) image: (H // m, W // m), not swapped, unless `lr_hw` names it."""
    H, W = (int(s) for s in size_hw)
    h, w = (H // m, W // m) if lr_hw is None else (int(s) for s in lr_hw)
    if h < 1 or w < 1 or h * m > H or w * m > W:
        raise ValueError(f"mtf: an LR image of {h}x{w} at magnification {m} does not fit {H}x{W}")
    return h, w


def _parse_list(text, bands, flag, check):
    if isinstance(text, numbers.Real) and not isinstance(text, bool):
        values = [float(text)]
    elif isinstance(text, str):
        try:
            values = [float(p) for p in text.split(",")]
        except ValueError:
            raise ValueError(f"{flag}={text!r}: expected a number or {bands} comma-separated numbers") from None
    else:
        try:
            values = [float(v) for v in text]
        except (TypeError, ValueError):
            raise ValueError(f"{flag}={text!r}: expected a number or {bands} numbers") from None
    bands = int(bands)
    if len(values) == 1:
        values = values * bands
    if len(values) != bands:
        raise ValueError(f"{flag}={text!r} names {len(values)} values, the images have {bands} bands (give one value, or one per band)")
    return tuple(check(v, flag) for v in values)


def _check_noise(s, what="mtf_noise"):
    if not (math.isfinite(s) and s >= 0):
        raise ValueError(f"{what}={s!r} must be a finite number >= 0 (a standard deviation in normalised units)")
    return float(s)


def parse_mtf_nyquist(text, bands):
    """--mtf_nyquist: "0.3" - one gain for all bands - or "0.35,0.35,0.34,0.26" - one per band -> a tuple of `bands` floats."""
    return _parse_list(text, bands, "--mtf_nyquist", _check_gain)


def parse_mtf_noise(text, bands):
    """--mtf_noise: per-band standard deviations >= 0 in normalised units, as `parse_mtf_nyquist`."""
    return _parse_list(text, bands, "--mtf_noise", _check_noise)


class DeviceMTFFeed:
    """Iterable of (lr, hr) fp32 batches drawn from a uint8 or uint16 HR cache (L, C, H, W) on the device under the MTF
    degradation, with the surface of `radiometry.DeviceU16SuperresFeed` (`__len__`, `__iter__`, `batch`, `item`, `epoch_order`,
    `last_items`) plus `operator` (the `consistency.BandOperator` of the same taps), `nyquist` and `noise`.  `nyquist`: one gain or
    one per band; `noise`: None, or per-band standard deviations in normalised units.  Every batch is one crop launch - a uint8
    cache / 255 (drs_crop_d4_u8_f32), a uint16 one through its `data_range` table, with the NaN-marked copy as the target under
    `nodata` (drs_crop_d4_u16_f32; `nodata` with a uint8 cache is refused) - and one `hip_ops.fir_decimate` of the stored pixels,
    clamped to [0, 1] and not quantised.  The normals of `noise` come from the feed's own device generator, seeded with (`seed`,
    `augment_rank`); a `fixed` feed (validation) seeds it again at every epoch and cuts centre windows; `item` adds no noise."""

    def __init__(self, cache, magnification_factor, nyquist, noise=None, batch_size=16, shuffle=True, data_range=None, nodata=None,
                 seed=0, fixed=False, crop_size=None, augment="none", num_crops=1, augment_seed=0, augment_rank=0, fixed_crop=False,
                 generator=None):
        from . import radiometry
        from .augment import FeedAugment
        from .consistency import BandOperator
        if not isinstance(cache, torch.Tensor) or cache.dtype not in (torch.uint8, torch.uint16) or cache.dim() != 4 or \
                cache.shape[0] < 1:
            raise RuntimeError("cache must be a non-empty (L, C, H, W) torch.uint8 or torch.uint16 tensor")
        self.hr = cache.contiguous()
        self.u16 = cache.dtype == torch.uint16
        L, c, H, W = self.hr.shape
        self.fixed = bool(fixed)
        self._aug = None
        if crop_size is not None or augment != "none" or fixed_crop:
            self._aug = FeedAugment(H, W, crop_size, augment, num_crops, augment_seed, augment_rank, fixed_crop or self.fixed)
        elif H != W:
            raise ValueError(f"the MTF feed takes square windows: give crop_size for scenes of {H} x {W}")
        self.size = self._aug.size if self._aug is not None else H
        self.last_items = None
        self.magnification_factor = _check_factor(magnification_factor)
        if self.size // self.magnification_factor < 1:
            raise ValueError(f"windows of {self.size} are too small for magnification {magnification_factor}")
        self.nyquist = parse_mtf_nyquist(nyquist, c)
        self.noise = None if noise is None else parse_mtf_noise(noise, c)
        self.batch_size, self.shuffle, self.generator = batch_size, shuffle, generator
        if self.u16:
            self.data_range = radiometry.check_table(
                radiometry.parse_data_range(radiometry.DEFAULT_RANGE)[1] * c if data_range is None else data_range, c)
            self.nodata = None if nodata is None else radiometry._check_u16("nodata", nodata)
        else:
            if nodata is not None:
                raise ValueError("nodata belongs to a uint16 cache (--bit_depth 16): the 8-bit MTF entrance has no no-data marker")
            if data_range is not None:
                raise ValueError("data_range belongs to a uint16 cache (--bit_depth 16)")
            self.data_range = self.nodata = None
        self.operator = BandOperator.mtf((self.size, self.size), self.magnification_factor, self.nyquist)
        self.taps, self.left, band_op = band_taps(self.nyquist, self.magnification_factor)
        assert band_op == self.operator.band_op
        self._seed = int(np.random.SeedSequence([int(seed), int(augment_rank)]).generate_state(1, dtype=np.uint64)[0] >> 1)
        self._device = None  # (taps, sigma, table, labels, generator) on the cache's device, made by the first batch

    def __len__(self):
        passes = self._aug.passes if self._aug is not None else 1
        return (passes * self.hr.shape[0] + self.batch_size - 1) // self.batch_size

    def _plain_items(self, src):
        src = np.asarray(src).reshape(-1)
        out = np.zeros((src.shape[0], 4), dtype=np.int32)
        out[:, 0] = src
        return out

    def _on_device(self):
        from . import radiometry
        dev = self.hr.device
        if self._device is None or self._device["device"] != dev:
            gen = torch.Generator(device=dev)
            gen.manual_seed(self._seed)
            self._device = {
                "device": dev, "generator": gen,
                "taps": torch.from_numpy(self.taps).to(torch.float32).to(dev).contiguous(),
                "sigma": None if self.noise is None else torch.tensor(self.noise, dtype=torch.float32, device=dev),
                "table": radiometry.device_table(self.data_range, dev) if self.u16 else None,
                "labels": None if self.u16 else torch.zeros(self.hr.shape[0], dtype=torch.int64, device=dev)}
        return self._device

    def batch(self, items, noisy=True):
        """(lr, hr or the marked hr) of the (n, 4) host items; `noisy` False leaves the sensor noise out."""
        from . import hip_ops, radiometry
        from .augment import crop_d4_u8_f32, upload_items
        d = self._on_device()
        on_device = upload_items(items, self.hr.device)
        if self.u16:
            hr, marked = radiometry.crop_d4_u16_f32(self.hr, on_device, self.size, d["table"], self.nodata)
        else:
            hr, marked = crop_d4_u8_f32(self.hr, d["labels"], on_device, self.size)[0], None
        z = None
        if noisy and self.noise is not None:
            lr_size = self.size // self.magnification_factor
            z = torch.randn((hr.shape[0], hr.shape[1], lr_size, lr_size), dtype=torch.float32, device=hr.device, generator=d["generator"])
        lr = hip_ops.fir_decimate(hr, d["taps"], d["taps"], self.left, self.magnification_factor, band_op=self.operator.band_op,
                                  noise=z, sigma=d["sigma"] if z is not None else None, clamp=True)
        return lr, (marked if self.nodata is not None else hr)

    def item(self, idx):
        """(lr, hr) of one dataset item, (C, h, w) / (C, S, S): the centre window (an active feed) or the whole image, no symmetry,
        no noise."""
        if not 0 <= idx < self.hr.shape[0]:
            raise IndexError(f"item {idx} of a dataset of {self.hr.shape[0]}")
        x, y = self.batch(self._aug.centre(idx) if self._aug is not None else self._plain_items([idx]), noisy=False)
        return x[0], y[0]

    def epoch_order(self):
        """The index vector of one epoch, on the host: `num_crops` orders, each drawn as one pass is."""
        n = self.hr.shape[0]

        def one_pass():
            return torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        return self._aug.epoch_order(one_pass) if self._aug is not None else one_pass()

    def __iter__(self):
        if self.fixed and self.noise is not None:
            self._on_device()["generator"].manual_seed(self._seed)  # the same noise every epoch
        order = self.epoch_order().numpy()
        for i in range(0, order.shape[0], self.batch_size):
            src = order[i:i + self.batch_size]
            self.last_items = self._aug.items(src) if self._aug is not None else self._plain_items(src)
            yield self.batch(self.last_items)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def add_mtf_args(p, in_help=True, noise=True):
    """--mtf_nyquist / --mtf_noise of the super-resolution trainer (`in_help` False: registered without a --help entry, like
    --prediction, because that help text is recorded), --mtf_nyquist alone of `evaluate` and the tiler."""
    import argparse
    p.add_argument("--mtf_nyquist", type=str, default=None,
                   help="the sensor-MTF degradation's gain at the LR Nyquist frequency, G (all bands) or G1,..,GC (one per band), "
                        f"each in {MIN_NYQUIST} .. {MAX_NYQUIST}; default: the snapshot's MTF_NYQUIST (a snapshot without it and "
                        "no flag: not an MTF run)" if in_help else argparse.SUPPRESS)
    if noise:
        p.add_argument("--mtf_noise", type=str, default=None,
                       help="with --Degradation_type MTF: the sensor noise's standard deviation in normalised units, S or "
                            "S1,..,SC" if in_help else argparse.SUPPRESS)
    return p


def is_mtf(args):
    return str(getattr(args, "Degradation_type", "") or "").lower() == "mtf"


def check_args(args):
    """ValueError, naming the flag, for a trainer command line that mixes the MTF degradation with what it does not have; sets
    `args.mtf_nyquist` / `args.mtf_noise` to the per-band tuples of an MTF run."""
    if not is_mtf(args):
        for flag in ("mtf_nyquist", "mtf_noise"):
            if getattr(args, flag, None) is not None:
                raise ValueError(f"--{flag} belongs to --Degradation_type MTF")
        return args
    bands = int(args.inp_out_channels)
    if getattr(args, "mtf_nyquist", None) is None:
        raise ValueError("--Degradation_type MTF needs --mtf_nyquist G or G1,..,GC: the gain at the LR Nyquist frequency")
    m = args.magnification_factor
    if m is None or not MIN_FACTOR <= int(m) <= MAX_FACTOR:
        raise ValueError(f"--magnification_factor {m} must lie in {MIN_FACTOR} .. {MAX_FACTOR} for --Degradation_type MTF")
    if str(getattr(args, "Blur_radius", "random")) != "random":
        raise ValueError("--Blur_radius belongs to the DownBlur degradations: --Degradation_type MTF blurs with --mtf_nyquist")
    spec = str(getattr(args, "dataset_path", None) or "")
    if spec.startswith("synthetic") and not spec.startswith(("synthetic_u8", "synthetic_u16")):
        raise ValueError(f"--dataset_path {spec!r}: the float DataLoader path has no degradation; --Degradation_type MTF reads an "
                         "image folder, synthetic_u8[:N] or, with --bit_depth 16, synthetic_u16[:N]")
    if getattr(args, "nodata", None) is not None and int(getattr(args, "bit_depth", 8) or 8) != 16:
        raise ValueError("--nodata with --Degradation_type MTF needs --bit_depth 16: the 8-bit MTF entrance has no no-data marker")
    args.mtf_nyquist = parse_mtf_nyquist(args.mtf_nyquist, bands)
    if getattr(args, "mtf_noise", None) is not None:
        args.mtf_noise = parse_mtf_noise(args.mtf_noise, bands)
    return args


def diffusion_kwargs(args):
    """The `Diffusion` keyword arguments of a checked command line: {} unless it is an MTF run."""
    if not is_mtf(args):
        return {}
    return {"mtf_nyquist": args.mtf_nyquist, "mtf_noise": getattr(args, "mtf_noise", None)}


def snapshot_nyquist(path):
    """The MTF_NYQUIST list of the snapshot at `path`, None for a file without the key or no file."""
    import os
    if not path or not os.path.exists(path):
        return None
    saved = torch.load(path, map_location="cpu").get("MTF_NYQUIST")
    return None if saved is None else tuple(float(g) for g in saved)


def resolve_nyquist(args, snapshot_path, bands):
    """`evaluate`'s and the tiler's --mtf_nyquist: the flag, else the snapshot's MTF_NYQUIST, else None (not an MTF run)."""
    flag = getattr(args, "mtf_nyquist", None)
    if flag is not None:
        return parse_mtf_nyquist(flag, bands)
    saved = snapshot_nyquist(snapshot_path)
    return None if saved is None else parse_mtf_nyquist(list(saved), bands)
