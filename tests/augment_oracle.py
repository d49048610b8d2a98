"""numpy restatement of the crop / dihedral augmentation of the device feeds, written from its
definition and not from the product: plain slicing, `swapaxes` and `[::-1]`.

Item i is `items[i] = (src, y0, x0, code)`: the S x S window of cache image `src` with top-left corner (y0, x0), then

    if code & 4: w = w.swapaxes(-1, -2)     # transpose first
    if code & 1: w = w[..., ::-1]           # then reverse the columns
    if code & 2: w = w[..., ::-1, :]        # then reverse the rows

An item is invalid when src is outside [0, L), the window does not lie inside H x W or code is outside 0..7: it reads nothing
and comes back as zeros (label -1)."""
import numpy as np

MODES = {"none": 1, "flip": 4, "d4": 8}


def d4(w, code):
    """The (..., S, S) array `w` under dihedral code 0..7."""
    if code & 4:
        w = w.swapaxes(-1, -2)
    if code & 1:
        w = w[..., ::-1]
    if code & 2:
        w = w[..., ::-1, :]
    return w


def is_valid(item, L, H, W, size):
    src, y0, x0, code = (int(v) for v in item)
    return 0 <= src < L and 0 <= code <= 7 and 0 <= y0 and y0 + size <= H and 0 <= x0 and x0 + size <= W


def crop_d4(cache, items, size):
    """(n, C, size, size) array of cache's dtype: the windows of `items` out of the (L, C, H, W) array `cache`; zeros for an
    invalid item."""
    cache, items = np.asarray(cache), np.asarray(items)
    L, C, H, W = cache.shape
    out = np.zeros((items.shape[0], C, size, size), dtype=cache.dtype)
    for i, item in enumerate(items):
        if is_valid(item, L, H, W, size):
            src, y0, x0, code = (int(v) for v in item)
            out[i] = d4(cache[src, :, y0:y0 + size, x0:x0 + size], code)
    return out


def crop_d4_u8_f32(cache, labels, items, size):
    """(float32(b) / float32(255) of the windows, labels[src] or -1): the class feed's form."""
    cache, labels, items = np.asarray(cache), np.asarray(labels), np.asarray(items)
    assert cache.dtype == np.uint8
    img = crop_d4(cache, items, size).astype(np.float32) / np.float32(255)
    L, _, H, W = cache.shape
    lab = np.array([labels[int(it[0])] if is_valid(it, L, H, W, size) else -1 for it in items], dtype=np.int64)
    return img, lab


def crop_d4_pairs(sar, ndvi, items, size):
    """((v + 1) * 0.5 of the windows of both fp32 caches, in float32; zeros for an invalid item): the SAR -> NDVI feed's form."""
    sar, ndvi, items = np.asarray(sar), np.asarray(ndvi), np.asarray(items)
    assert sar.dtype == ndvi.dtype == np.float32 and sar.shape[0] == ndvi.shape[0] and sar.shape[2:] == ndvi.shape[2:]
    L, _, H, W = sar.shape
    ok = np.array([is_valid(it, L, H, W, size) for it in items]).reshape(-1, 1, 1, 1)
    outs = []
    for cache in (sar, ndvi):
        w = crop_d4(cache, items, size)
        outs.append(np.where(ok, (w + np.float32(1)) * np.float32(0.5), np.float32(0)).astype(np.float32))
    return outs[0], outs[1]


def draw_items(rng, src, H, W, size, augment):
    """(n, 4) int32: the n codes, then the n row offsets, then the n column offsets from `rng`, in this order."""
    src = np.asarray(src).reshape(-1)
    n = src.shape[0]
    code = rng.integers(0, MODES[augment], n)
    y0 = rng.integers(0, H - size + 1, n)
    x0 = rng.integers(0, W - size + 1, n)
    return np.stack([src, y0, x0, code], axis=1).astype(np.int32)


def centre_items(src, H, W, size):
    """(n, 4) int32: the centre window, code 0."""
    src = np.asarray(src).reshape(-1)
    out = np.zeros((src.shape[0], 4), dtype=np.int32)
    out[:, 0] = src
    out[:, 1] = (H - size) // 2
    out[:, 2] = (W - size) // 2
    return out
