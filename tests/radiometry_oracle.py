"""numpy restatement of the 16-bit radiometry, written from its definition and not from the product.

A band's range is (lo, hi), fp32.  Every step is one fp32 operation on float32 arrays (numpy rounds each correctly and never
contracts two into one):

    normalise   x = min(max((float32(v) - lo) / (hi - lo), 0), 1)
    quantise    v = clamp(rint(min(max(x, 0), 1) * (hi - lo) + lo), 0, 65535), np.rint rounds half to even, NaN -> fill

A pixel is no-data when ALL its stored band values equal `nodata`; the comparison is on the integers."""
import numpy as np

import augment_oracle as AO

F = np.float32


def _cols(table, ndim, band_axis):
    t = np.asarray(table, dtype=F)
    shape = [1] * ndim
    shape[band_axis] = -1
    lo, hi = t[:, 0].reshape(shape), t[:, 1].reshape(shape)
    span = hi - lo  # float32 - float32: formed once
    assert span.dtype == F and lo.dtype == F
    return lo, span


def normalise(v, table, band_axis=0):
    v = np.asarray(v)
    lo, span = _cols(table, v.ndim, band_axis)
    d = v.astype(F) - lo
    q = d / span
    assert d.dtype == F and q.dtype == F
    return np.minimum(np.maximum(q, F(0)), F(1))


def quantize(x, table, fill=0, band_axis=0):
    x = np.asarray(x, dtype=F)
    lo, span = _cols(table, x.ndim, band_axis)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(np.where(nan, F(0), x), F(0)), F(1))
        p = c * span
        s = p + lo
        assert p.dtype == F and s.dtype == F
        v = np.minimum(np.maximum(np.rint(s), F(0)), F(65535)).astype(np.uint16)
    return np.where(nan, np.uint16(fill), v)


def nodata_pixels(cache, nodata):
    """(L, 1, H, W) bool: the pixels of a (L, C, H, W) integer cache whose bands all equal `nodata` (None: none)."""
    cache = np.asarray(cache)
    if nodata is None:
        return np.zeros((cache.shape[0], 1) + cache.shape[2:], dtype=bool)
    return (cache == nodata).all(axis=1, keepdims=True)


def crop_mark(cache, items, size, table, nodata=None):
    """(hr, hr_marked): the windows of `items` (augment_oracle.crop_d4) normalised, and the same with NaN in all bands of every
    no-data pixel; an invalid item is zeros in both."""
    cache, items = np.asarray(cache), np.asarray(items)
    assert cache.dtype == np.uint16
    L, C, H, W = cache.shape
    ok = np.array([AO.is_valid(it, L, H, W, size) for it in items]).reshape(-1, 1, 1, 1)
    dn = AO.crop_d4(cache, items, size)
    hr = np.where(ok, normalise(dn, table, band_axis=1), F(0)).astype(F)
    nd = AO.crop_d4(np.broadcast_to(nodata_pixels(cache, nodata), cache.shape).astype(np.uint8), items, size).astype(bool)
    return hr, np.where(nd & ok, F(np.nan), hr).astype(F)


def histogram(cache, nodata=None):
    """(C, 65536) int64: np.bincount per band over the pixels that are not no-data."""
    cache = np.asarray(cache)
    assert cache.dtype == np.uint16
    keep = ~nodata_pixels(cache, nodata)[:, 0]
    return np.stack([np.bincount(cache[:, c][keep].astype(np.int64), minlength=65536) for c in range(cache.shape[1])]).astype(np.int64)


def range_from_counts(counts, plo, phi):
    """(C, 2) float32: per band the values of 0-based rank floor(p / 100 (n - 1)) of the sorted counted pixels."""
    out = []
    for row in np.asarray(counts):
        values = np.repeat(np.arange(65536), row)  # the band's counted pixels, sorted
        out.append([values[int(np.floor(p / 100 * (values.size - 1)))] for p in (plo, phi)])
    return np.asarray(out, dtype=F)
