"""The three launches of csrc/radiometry.hip, the 16-bit feed and the command lines that use it (diffusionremotesensing_amd/
radiometry.py) against the numpy oracle (tests/radiometry_oracle.py).

Every output element of the crop and of the quantiser is a chain of correctly rounded fp32 operations that numpy performs
alike, and the histogram counts integers: the bar for all three is equality of bits.  The feed's LR image is a product of fp32
matrices and is held to the float64 operator within the bar tests/test_gpu_consistency.py uses for `degrade`.

Shapes: the crop takes tests/test_gpu_augment.py's six (odd sizes, odd offsets, pitches that are no multiple of 4, ragged and
whole 64-tiles, 16 bands) and its 24 items; the histogram's caches reach one pixel, planes shorter than a 16-byte vector, a
chunk that spans several planes, more than one 65280-pixel chunk per band, a constant plane (the wave-uniform add) and a
pointer on an odd element."""
import json
import math
import os

import numpy as np
import pytest
import torch

import consistency_oracle as CO
import radiometry_oracle as RO
import test_gpu_augment as GA
import test_gpu_consistency as GC

pytestmark = pytest.mark.gpu

K = 777  # the no-data value of the cases that have one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _table(bands):
    return np.array([(123 + 10 * c, 4567 + 100 * c) for c in range(bands)], dtype=np.float32)


def _u16_cache(shape, seed, length=GA.L, nodata=None):
    """(L, C, H, W) uint16, seeded: 70 % of the values around the bands' ranges, the rest anywhere in 0 .. 65535, with 0, 65535
    and every band's lo - 1, lo, hi, hi + 1 among them, shuffled.  With `nodata`: about 5 % of the pixels hold it in all bands
    and (C > 1) about 5 % in band 0 alone."""
    c, H, W = shape
    n = length * c * H * W
    rng = np.random.default_rng(seed)
    v = np.where(rng.random(n) < 0.7, rng.integers(100, 5000, n), rng.integers(0, 65536, n))
    special = [0, 65535] + [int(x) + d for lo, hi in _table(c) for x, d in ((lo, -1), (lo, 0), (hi, 0), (hi, 1))]
    if n >= len(special):
        v[:len(special)] = special
    else:
        v[:] = special[:n]
    cache = rng.permutation(v).astype(np.uint16).reshape(length, c, H, W)
    if nodata is not None:
        cache[cache == nodata] += 1
        draw = rng.random((length, H, W))
        cache[:, 0][(draw >= 0.05) & (draw < 0.10)] = nodata  # band 0 alone (C == 1: that is all bands)
        cache[np.broadcast_to((draw < 0.05)[:, None], cache.shape)] = nodata
        free = np.nonzero((draw >= 0.10).reshape(-1))[0][:len(special)]  # the special values again, where the planting left room
        band0 = cache[:, 0].reshape(-1)
        band0[free] = special[:free.size]
        cache[:, 0] = band0.reshape(length, H, W)
    return torch.from_numpy(cache)


def _odd_view(cache, dev):
    """`cache` on the device as a view that starts on the second element of its buffer: the 2-byte pointer phase."""
    host = torch.from_numpy(np.concatenate([[1], cache.numpy().reshape(-1)]).astype(np.uint16))  # (assembled on the host)
    return host.to(dev)[1:].view(cache.shape)


def _same_bits(got, want, what):
    got, want = got.cpu().numpy(), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    view = {4: np.uint32, 2: np.uint16, 8: np.uint64}[got.dtype.itemsize]
    bad = np.nonzero(got.view(view).reshape(-1) != want.view(view).reshape(-1))[0]
    assert bad.size == 0, (what, f"{bad.size} of {got.size} elements differ, the first at {int(bad[0])}: "
                           f"{got.reshape(-1)[bad[0]]!r} against {want.reshape(-1)[bad[0]]!r}")


def _same_marked(got, want, what):
    g, w = got.cpu().numpy(), np.ascontiguousarray(want)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions")
    _same_bits(torch.from_numpy(np.nan_to_num(g, nan=-1.0)), np.nan_to_num(w, nan=-1.0), what)


# ---------------------------------------------------------------------------------------------
# crop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GA.SHAPES)
def test_crop_bit_exact(dev, shape):
    from diffusionremotesensing_amd import radiometry as R
    c, H, W, S = shape
    items = GA._items(H, W, S)
    assert len(items) == 24
    table = _table(c)
    cache = _u16_cache((c, H, W), 80 + c + H, nodata=K)
    present = set(np.unique(cache.numpy()).tolist())
    if cache.numel() >= 200:
        assert {0, 65535, 122, 123, 4567, 4568} <= present
    want_hr, want_marked = RO.crop_mark(cache.numpy(), items, S, table, K)
    if S >= 9:  # (the 3 x 3 windows of the tiny case need not meet one)
        assert np.isnan(want_marked).any() and (want_hr == 0).any() and (want_hr == 1).any()
    hr, marked = R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, R.device_table(table, dev), nodata=K)
    assert hr.dtype == marked.dtype == torch.float32 and tuple(hr.shape) == (24, c, S, S)
    _same_bits(hr, want_hr, ("hr", shape))
    _same_marked(marked, want_marked, ("hr_marked", shape))
    # without a no-data value: one output, the same values
    plain, none = R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, R.device_table(table, dev))
    assert none is None
    _same_bits(plain, want_hr, ("hr without nodata", shape))
    # ... and marked=True without a value writes the second output unmarked
    _, unmarked = R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, R.device_table(table, dev), marked=True)
    _same_bits(unmarked, want_hr, ("hr_marked without nodata", shape))


def test_crop_at_an_odd_element(dev):
    """The cache pointer on a 2-byte phase: every row that was 8-byte aligned is not, and the reverse."""
    from diffusionremotesensing_amd import radiometry as R
    c, H, W, S = GA.SHAPES[2]
    items, table = GA._items(H, W, S), _table(c)
    cache = _u16_cache((c, H, W), 5, nodata=K)
    view = _odd_view(cache, dev)
    assert view.data_ptr() % 4 == 2 and view.is_contiguous()
    hr, marked = R.crop_d4_u16_f32(view, torch.from_numpy(items).to(dev), S, R.device_table(table, dev), nodata=K)
    want_hr, want_marked = RO.crop_mark(cache.numpy(), items, S, table, K)
    _same_bits(hr, want_hr, "hr")
    _same_marked(marked, want_marked, "hr_marked")


def test_nodata_needs_all_bands(dev):
    """Pixels whose bands all equal K are marked in all bands; pixels where only some do stay valid, in every band."""
    from diffusionremotesensing_amd import radiometry as R
    c, H, W, S = 3, 20, 24, 20
    cache = _u16_cache((c, H, W), 9).numpy().copy()
    cache[cache == K] += 1
    cache[:, :, 3, 5] = K              # all bands
    cache[:, 0, 7, 7] = K              # one band
    cache[:, 1:, 9, 11] = K            # all but one
    cache[1, :, 0, 0] = K              # image 1 only
    items = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 4, 6]], dtype=np.int32)
    table = _table(c)
    hr, marked = R.crop_d4_u16_f32(torch.from_numpy(cache).to(dev), torch.from_numpy(items).to(dev), S, R.device_table(table, dev),
                                   nodata=K)
    want_hr, want_marked = RO.crop_mark(cache, items, S, table, K)
    _same_bits(hr, want_hr, "hr")
    _same_marked(marked, want_marked, "hr_marked")
    nan = torch.isnan(marked).cpu()
    assert bool((nan.all(dim=1) == nan.any(dim=1)).all())  # a pixel is marked in all bands or in none
    assert nan[0, :, 3, 5].all() and not nan[0, :, 7, 7].any() and not nan[0, :, 9, 11].any() and not nan[0, :, 0, 0].any()
    assert nan[1, :, 3, 5].all() and nan[1, :, 0, 0].all()
    assert int(nan[2, 0].sum()) == 1  # image 2 under code 6 at x0 = 4: its one no-data pixel, wherever the symmetry puts it
    assert int(nan[:, 0].sum()) == int(np.isnan(want_marked[:, 0]).sum())
    assert not torch.isnan(hr).any()


def test_invalid_items_give_zeros(dev):
    from diffusionremotesensing_amd import radiometry as R
    import augment_oracle as AO
    c, H, W, S = 2, 40, 72, 33
    L = GA.L
    items = np.array([[1, 3, 5, 6], [L, 0, 0, 0], [0, H - S, W - S, 3], [-1, 0, 0, 0], [2, H - S + 1, 0, 0], [2, 0, -1, 1],
                      [1, 0, 0, 8], [1, 0, 0, -1], [2, 1, 2, 7], [0, -1, 0, 4], [0, 0, W - S + 1, 5], [2, 7, 39, 4]], dtype=np.int32)
    ok = [AO.is_valid(it, L, H, W, S) for it in items]
    assert ok == [True, False, True, False, False, False, False, False, True, False, False, True]
    cache, table = _u16_cache((c, H, W), 3, nodata=K), _table(c)
    hr, marked = R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, R.device_table(table, dev), nodata=K)
    want_hr, want_marked = RO.crop_mark(cache.numpy(), items, S, table, K)
    _same_bits(hr, want_hr, "hr")
    _same_marked(marked, want_marked, "hr_marked")
    for i, valid in enumerate(ok):
        if not valid:
            assert not hr[i].any() and not marked[i].any()
    with pytest.raises(RuntimeError, match="does not fit"):
        R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), 41, R.device_table(table, dev))
    with pytest.raises(RuntimeError, match=r"\(2, 2\) float32"):
        R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, R.device_table(_table(3), dev))


# ---------------------------------------------------------------------------------------------
# histogram
# ---------------------------------------------------------------------------------------------
def _hist_cache(name):
    rng = np.random.default_rng(21)
    if name == "one pixel":
        return np.array([[[[4242]]]], dtype=np.uint16)
    if name == "(2, 3, 5, 7)":
        return _u16_cache((3, 5, 7), 22, length=2).numpy()
    if name == "(3, 16, 16, 16)":
        return _u16_cache((16, 16, 16), 23, length=3).numpy()
    if name == "every value once":
        return rng.permutation(65536).astype(np.uint16).reshape(1, 1, 256, 256)
    if name == "a constant plane":
        cache = rng.integers(0, 65536, (1, 2, 64, 130)).astype(np.uint16)
        cache[0, 1] = 31337
        return cache
    if name == "a chunk boundary inside a plane":  # (added) 5 x 15600 = 78000 pixels per band: the second chunk starts in image 4
        cache = np.minimum(rng.gamma(2.0, 200.0, (5, 2, 120, 130)), 65535).astype(np.uint16)  # a few hundred values carry the band
        cache[:, 1] = 9
        return cache
    raise KeyError(name)


HIST_CASES = ["one pixel", "(2, 3, 5, 7)", "(3, 16, 16, 16)", "every value once", "a constant plane",
              "a chunk boundary inside a plane"]


@pytest.mark.parametrize("name", HIST_CASES)
def test_histogram_is_bincount(dev, name):
    from diffusionremotesensing_amd import radiometry as R
    cache = _hist_cache(name)
    want = RO.histogram(cache)
    assert want.sum() == cache.size
    got = R.hist_u16(torch.from_numpy(cache).to(dev))
    assert got.dtype == torch.int64 and tuple(got.shape) == (cache.shape[1], 65536)
    _same_bits(got, want, name)
    _same_bits(R.hist_u16(torch.from_numpy(cache).to(dev)), got.cpu().numpy(), "a second run")


@pytest.mark.parametrize("name", ["(2, 3, 5, 7)", "a constant plane", "a chunk boundary inside a plane"])
def test_histogram_at_an_odd_element(dev, name):
    from diffusionremotesensing_amd import radiometry as R
    cache = torch.from_numpy(_hist_cache(name))
    view = _odd_view(cache, dev)
    assert view.data_ptr() % 4 == 2
    _same_bits(R.hist_u16(view), RO.histogram(cache.numpy()), name)


@pytest.mark.parametrize("bands", [1, 3])
def test_histogram_skips_nodata_pixels(dev, bands):
    from diffusionremotesensing_amd import radiometry as R
    cache = _u16_cache((bands, 33, 47), 31, length=2, nodata=K)
    if bands > 1:
        assert int((cache[:, 0] == K).sum()) > int((cache == K).all(dim=1).sum()) > 0
    want = RO.histogram(cache.numpy(), K)
    assert want.sum() < cache.numel() and (want.sum(axis=1) == want.sum(axis=1)[0]).all()
    _same_bits(R.hist_u16(cache.to(dev), nodata=K), want, "nodata")
    _same_bits(R.hist_u16(cache.to(dev)), RO.histogram(cache.numpy()), "no nodata")
    # a no-data region as scenes have it: a whole corner, contiguous
    cache = cache.numpy().copy()
    cache[:, :, :20, :30] = 0
    _same_bits(R.hist_u16(torch.from_numpy(cache).to(dev), nodata=0), RO.histogram(cache, 0), "a corner of zeros")
    table = R.auto_range(torch.from_numpy(cache).to(dev), 2.0, 98.0, nodata=0)
    assert table.tolist() == RO.range_from_counts(RO.histogram(cache, 0), 2.0, 98.0).tolist()


# ---------------------------------------------------------------------------------------------
# quantize
# ---------------------------------------------------------------------------------------------
def test_quantize_round_trip_grids(dev):
    """All 65536 values through normalise (oracle) and the device quantiser, at the three ranges, one per band."""
    from diffusionremotesensing_amd import radiometry as R
    table = np.array([(0, 65535), (0, 10000), (123, 4567)], dtype=np.float32)
    dn = np.broadcast_to(np.arange(65536, dtype=np.uint16).reshape(1, 1, 256, 256), (1, 3, 256, 256))
    x = RO.normalise(dn, table, band_axis=1)
    got = R.quantize_u16(torch.from_numpy(x).to(dev), R.device_table(table, dev))
    assert got.dtype == torch.uint16
    _same_bits(got, RO.quantize(x, table, band_axis=1), "grids")
    for c, (lo, hi) in enumerate(table.astype(int)):
        assert np.array_equal(got[0, c].cpu().numpy().reshape(-1), np.clip(np.arange(65536), lo, hi).astype(np.uint16))


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 1, 1), (3, 16, 8, 8), (1, 1, 33, 47)], ids=str)
def test_quantize_bit_exact(dev, shape):
    """Random values in [-0.2, 1.2] with the half-way cases, NaN, +-inf and -0.0 planted, H W % 4 != 0 (a group of four straddles
    two bands) and == 0, at the three pointer phases a fp32 / uint16 pair can have."""
    from diffusionremotesensing_amd import radiometry as R
    n, c, H, W = shape
    table = np.array([(0, 4), (7, 11), (123, 4567), (0, 65535)] * 4, dtype=np.float32)[:c]
    rng = np.random.default_rng(sum(shape))
    x = (rng.random(shape) * 1.4 - 0.2).astype(np.float32)
    special = np.array([0.125, 0.375, 0.625, 0.875, np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.5], dtype=np.float32)
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)[:min(4 * special.size, flat.size)]
    flat[pos] = np.resize(special, pos.size)
    want = RO.quantize(x, table, fill=999, band_axis=1)
    td = R.device_table(table, dev)
    _same_bits(R.quantize_u16(torch.from_numpy(x).to(dev), td, fill=999), want, shape)
    shifted = torch.from_numpy(np.concatenate([[0], x.reshape(-1)]).astype(np.float32)).to(dev)
    _same_bits(R.quantize_u16(shifted[1:].view(shape), td, fill=999), want, (shape, "x at +4 bytes"))
    with pytest.raises(ValueError, match="fill"):
        R.quantize_u16(torch.from_numpy(x).to(dev), td, fill=-1)


def test_quantize_inverts_the_crop(dev):
    """quantise(normalise(v)) == v on the device, for the values inside their band's range."""
    from diffusionremotesensing_amd import radiometry as R
    c, H, W, S = GA.SHAPES[1]
    cache, table = _u16_cache((c, H, W), 41), _table(c)
    items = np.array([[i, 0, 0, 0] for i in range(GA.L)], dtype=np.int32)
    td = R.device_table(table, dev)
    hr, _ = R.crop_d4_u16_f32(cache.to(dev), torch.from_numpy(items).to(dev), S, td)
    back = R.quantize_u16(hr, td).cpu().numpy()
    lo, hi = table[:, 0].reshape(1, c, 1, 1), table[:, 1].reshape(1, c, 1, 1)
    assert np.array_equal(back, np.clip(cache.numpy(), lo, hi).astype(np.uint16))


# ---------------------------------------------------------------------------------------------
# the feed
# ---------------------------------------------------------------------------------------------
def _scenes():
    """(6, 3, 48, 48) uint16 in 3000 .. 7000: under the range 0,10000 the clamp of the LR image is never active."""
    rng = np.random.default_rng(77)
    return torch.from_numpy(rng.integers(3000, 7001, (6, 3, 48, 48)).astype(np.uint16))


def test_feed(dev):
    from diffusionremotesensing_amd import consistency
    from diffusionremotesensing_amd import radiometry as R
    scenes, table = _scenes(), np.array([(0, 10000)] * 3, dtype=np.float32)
    feed = R.DeviceU16SuperresFeed(scenes.to(dev), 2, 0.5, 4, True, table, crop_size=32, augment="d4", num_crops=2, augment_seed=3,
                                   generator=torch.Generator().manual_seed(1))
    assert len(feed) == 3 and feed.blur_radius == 0.5
    A_y, A_x = CO.downblur_matrices(32, 32, 2, 0.5)
    assert np.allclose(feed.operator.A_y, A_y, rtol=0, atol=1e-15) and np.allclose(feed.operator.A_x, A_x, rtol=0, atol=1e-15)
    seen = 0
    for lr, hr in feed:
        items = feed.last_items
        n = items.shape[0]
        assert items.dtype == np.int32 and items.shape == (n, 4) and tuple(hr.shape) == (n, 3, 32, 32) and tuple(lr.shape) == (n, 3, 16, 16)
        want_hr, _ = RO.crop_mark(scenes.numpy(), items, 32, table)
        _same_bits(hr, want_hr, "hr")  # `last_items` are the windows of this batch
        want = feed.operator.apply(want_hr.astype(np.float64))  # float64 A_y hr A_x^T, un-clamped
        assert want.min() > 0.05 and want.max() < 0.95          # the clamp is inactive
        bound = CO.gamma(32, 32, 16, 16) * (np.abs(A_y) @ np.abs(want_hr.astype(np.float64)) @ np.abs(A_x).T)
        GC._within(lr, (want, bound), "lr")
        rm = consistency.lr_rmse(hr, lr, feed.operator)
        GC._within(rm, (np.zeros(n), np.sqrt((bound ** 2).mean(axis=(1, 2, 3)))), "lr_rmse of the truth")
        seen += n
    assert seen == 12
    # the validation feed: centre windows, no symmetry, the same batches in every epoch
    val = R.DeviceU16SuperresFeed(scenes.to(dev), 2, 0.5, 4, False, table, crop_size=32, fixed_crop=True)
    first, second = [(lr.clone(), hr.clone(), val.last_items.copy()) for lr, hr in val], [(lr, hr, val.last_items) for lr, hr in val]
    assert len(first) == len(second) == 2
    for (lr1, hr1, it1), (lr2, hr2, it2) in zip(first, second):
        assert GC.bits_equal(lr1, lr2) and GC.bits_equal(hr1, hr2) and np.array_equal(it1, it2)
        assert (it1[:, 1:] == [8, 8, 0]).all()
    x, y = val.item(4)
    assert GC.bits_equal(x, first[1][0][0]) and GC.bits_equal(y, first[1][1][0])
    # without crops: the item (idx, 0, 0, 0) at the cache's own size
    whole = R.DeviceU16SuperresFeed(scenes.to(dev), 2, 0.5, 4, False, table)
    lr, hr = next(iter(whole))
    assert whole.last_items.tolist() == [[i, 0, 0, 0] for i in range(4)] and tuple(hr.shape) == (4, 3, 48, 48)
    _same_bits(hr, RO.normalise(scenes.numpy()[:4], table, band_axis=1), "whole images")
    # with a no-data value the feed yields the marked target; the LR image is made from the stored pixels
    holes = scenes.clone().numpy()
    holes[:, :, 10:14, 20:30] = 0
    marked_feed = R.DeviceU16SuperresFeed(torch.from_numpy(holes).to(dev), 2, 0.5, 4, False, table, nodata=0)
    lr_m, hr_m = next(iter(marked_feed))
    assert torch.isnan(hr_m[:, :, 10:14, 20:30]).all() and int(torch.isnan(hr_m).sum()) == 4 * 3 * 40 and torch.isfinite(lr_m).all()


def test_the_8_bit_feed_calls_no_new_entry(dev, monkeypatch):
    """A default run launches what it launched: the feeds `make_superres_feeds` builds without --bit_depth 16 give the bits of
    `degradation.downblur` on the cache and never fetch one of the three new entries (recording proxy of tests/guard.py)."""
    import guard
    from diffusionremotesensing_amd import _lib
    from diffusionremotesensing_amd import train_diffusion_superres as T
    from diffusionremotesensing_amd.degradation import DeviceSuperresFeed, downblur
    from diffusionremotesensing_amd.superres_feeds import make_superres_feeds
    args = T.parse_train_args(["--image_size", "16", "--batch_size", "2", "--dataset_path", "synthetic_u8:4", "--magnification_factor", "2",
                               "--Blur_radius", "0.5", "--scene_size", "32", "--augment", "flip"])
    assert args.bit_depth == 8 and args.data_range is None
    calls, real_load = set(), _lib.load
    monkeypatch.setattr(_lib, "load", lambda: guard._RecordingLib(real_load(), calls))
    train, val, final_lr = make_superres_feeds(args, dev)
    assert type(train) is DeviceSuperresFeed and type(val) is DeviceSuperresFeed and train.hr.dtype == torch.uint8
    for feed in (train, val):
        for lr, hr in feed:
            from diffusionremotesensing_amd.augment import crop_d4_u8, upload_items
            want = downblur(crop_d4_u8(feed.hr, upload_items(feed.last_items, dev), 16), 2, 0.5)
            assert GC.bits_equal(lr, want[0]) and GC.bits_equal(hr, want[1])
    assert {"drs_downblur_u8", "drs_crop_d4_u8"} <= calls
    assert not calls & {"drs_hist_u16", "drs_crop_d4_u16_f32", "drs_quantize_u16"}, calls


# ---------------------------------------------------------------------------------------------
# end to end, at the smallest shape the network takes
# ---------------------------------------------------------------------------------------------
_EVAL = GA._RUN + ["--dataset_path", "synthetic_u16:8", "--bit_depth", "16", "--scene_size", "32", "--nodata", "0",
                   "--magnification_factor", "2", "--Blur_radius", "0.5"]
_RUN = _EVAL + ["--augment", "d4"]


def test_trainer_and_evaluate(dev, tmp_path, monkeypatch, capsys):
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import radiometry as R
    from diffusionremotesensing_amd import train_diffusion_superres as T
    from diffusionremotesensing_amd.superres_feeds import SyntheticSuperresDataset
    monkeypatch.chdir(tmp_path)
    losses, inner = [], T.Diffusion.train_step

    def recorded(self, *args, **kwargs):
        loss = inner(self, *args, **kwargs)
        losses.append(float(loss))
        return loss
    monkeypatch.setattr(T.Diffusion, "train_step", recorded)
    torch.manual_seed(0)
    T.main(_RUN + ["--model_name", "sr16", "--data_range", "auto"])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Training snapshot saved" in out and "16-bit radiometry: band ranges" in out
    assert len(losses) == 4 and all(math.isfinite(v) for v in losses), losses
    snapshot = torch.load(tmp_path / "models_run" / "sr16" / "weights" / "snapshot.pt")
    # the percentiles of the training scenes, from the oracle
    scenes = R.synthetic_u16(SyntheticSuperresDataset(8, 3, 32, 2, seed=1).hr).numpy()
    want = RO.range_from_counts(RO.histogram(scenes, 0), 0.5, 99.5)
    assert snapshot["DATA_RANGE"].dtype == torch.float32 and snapshot["DATA_RANGE"].tolist() == want.tolist()
    res = torch.load(tmp_path / "models_run" / "sr16" / "results" / "superres_results.pt")
    assert tuple(res.shape) == (5, 3, 16, 16) and bool(torch.isfinite(res).all())
    # evaluate reads the table from the snapshot
    scores = evaluate.main(_EVAL + ["--model_name", "sr16", "--n_images", "2", "--sampling_steps", "4", "--out", str(tmp_path / "scores.json")])
    out = capsys.readouterr().out
    assert f"16-bit radiometry: band ranges {R.format_table(want)}" in out
    assert scores["n"] == 2 and "valid_fraction" in scores["model"] and 0.99 <= scores["model"]["valid_fraction"] <= 1.0
    assert all(math.isfinite(v) for v in scores["model"].values()), scores["model"]
    assert "valid_fraction" in json.load(open(tmp_path / "scores.json"))["model"]
    # a resume under other band ranges is refused
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --data_range .*, this run has 0,10000;0,10000;0,10000"):
        T.main(_RUN + ["--model_name", "sr16", "--data_range", "0,10000"])


def test_tiler_reads_and_writes_digital_numbers(dev, tmp_path, monkeypatch):
    """The tiler's uint16 entrance and exit, without a network: `launch` normalises a uint16 scene with the snapshot's table and
    `--out_u16` writes what the quantiser makes of the returned scene."""
    from diffusionremotesensing_amd import Aggregation_Sampling as A
    from diffusionremotesensing_amd import radiometry as R
    from diffusionremotesensing_amd import train_diffusion_superres as T
    table = np.array([(0, 10000), (100, 5000), (50, 60000)], dtype=np.float32)
    dn = _u16_cache((3, 8, 8), 51, length=1)[0].numpy()
    np.save(tmp_path / "lr.npy", dn)
    seen = {}

    class Tiler:
        def __init__(self, img_lr, *a, **kw):
            seen["lr"] = img_lr

        def aggregation_sampling(self, **kw):
            return seen["lr"].clone()  # "super-resolve" by handing the normalised scene back
    monkeypatch.setattr(A, "split_aggregation_sampling", Tiler)
    monkeypatch.setattr(T.Diffusion, "_load_snapshot", lambda self: setattr(self, "snapshot_data_range", torch.from_numpy(table)))
    os.makedirs(tmp_path / "w")
    torch.save({}, tmp_path / "w" / "snapshot.pt")
    args = A.build_arg_parser().parse_args(["--model_name", "x", "--UNet_type", "Residual Attention UNet", "--Degradation_type", "DownBlur",
                                            "--magnification_factor", "2", "--model_input_size", "16", "--noise_steps", "10",
                                            "--img_lr_path", str(tmp_path / "lr.npy"), "--destination_path", str(tmp_path / "out.npy"),
                                            "--out_u16", "--device", "cuda:0"])
    args.snapshot_folder_path = str(tmp_path / "w")
    A.launch(args)
    _same_bits(seen["lr"][0], RO.normalise(dn, table), "the normalised scene")
    out = np.load(tmp_path / "out.npy")
    assert out.dtype == np.uint16 and np.array_equal(out, RO.quantize(RO.normalise(dn, table), table))
    lo, hi = table[:, 0].reshape(3, 1, 1), table[:, 1].reshape(3, 1, 1)
    assert np.array_equal(out, np.clip(dn, lo, hi).astype(np.uint16))
