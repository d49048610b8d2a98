"""The crop / dihedral kernels of csrc/augment.hip and the four device feeds with `crop_size` / `augment` set
(diffusionremotesensing_amd/augment.py), bit for bit against the numpy oracle (tests/augment_oracle.py):
every output element is a copy or one correctly rounded fp32 operation, so the bar is equality.  Then one epoch of the SAR ->
NDVI and the super-resolution trainers on windows of larger scenes.

The kernel's tile is 64 x 64 outputs; its two lane mappings and its vector / element paths are chosen by the alignment of the
window's rows and of the output rows, which the shapes below vary (odd sizes, odd offsets, pitches that are no multiple of 4)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import augment_oracle as O
from feeds_fixtures import write_sar_folder

pytestmark = pytest.mark.gpu

L = 3
#         C   H   W   S
SHAPES = [(1, 5, 7, 3),      # tiny, every row unaligned, odd S
          (3, 9, 9, 9),      # window = whole image, S no multiple of 4
          (2, 40, 72, 33),   # a ragged tile, H != W
          (1, 80, 96, 70),   # more than one 64-tile per side with a ragged second tile
          (16, 16, 16, 16),  # 16 bands, everything aligned
          (1, 132, 136, 128)]  # (added to the issue's list) two full tiles per side on the vector paths of both sides
FORMS = ("u8", "u8_f32", "pairs")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _u8_cache(shape, seed, length=L):
    """(L, C, H, W) uint8: a seeded shuffle of 0, 1, 2, ... (mod 256), so every byte value occurs once there are 256 elements."""
    n = length * shape[0] * shape[1] * shape[2]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return (torch.arange(n)[perm] % 256).to(torch.uint8).view((length,) + shape)


def _f32_cache(shape, seed, length=L):
    """(L, C, H, W) fp32 in [-1.5, 1.5] with the exact values -1, 0 and 1."""
    x = torch.rand((length,) + shape, generator=torch.Generator().manual_seed(seed)) * 3 - 1.5
    x.view(length, -1)[:, :3] = torch.tensor([-1.0, 0.0, 1.0])
    return x


def _items(H, W, S):
    """24 items: the 8 codes at the offsets (0, 0), (H - S, W - S) and an odd one; src cycles through 2, 1, 0."""
    offsets = [(0, 0), (H - S, W - S), (min(1, H - S), min(2, W - S))]
    rows = [(y0, x0, code) for (y0, x0) in offsets for code in range(8)]
    return np.array([(2 - i % 3, y0, x0, code) for i, (y0, x0, code) in enumerate(rows)], dtype=np.int32)


def _run(form, dev, shape, items, seed=0):
    """(what the launch gave, what the oracle gives) as tuples of host tensors, for one entry point."""
    from diffusionremotesensing_amd.augment import crop_d4_pairs, crop_d4_u8, crop_d4_u8_f32
    c, H, W, S = shape
    items_d = torch.from_numpy(items).to(dev)
    if form == "pairs":
        sar, ndvi = _f32_cache((2, H, W), 60 + seed), _f32_cache((1, H, W), 70 + seed)
        got = crop_d4_pairs(sar.to(dev), ndvi.to(dev), items_d, S)
        want = O.crop_d4_pairs(sar.numpy(), ndvi.numpy(), items, S)
        assert got[0].shape == (len(items), 2, S, S) and got[1].shape == (len(items), 1, S, S)
    else:
        u8 = _u8_cache((c, H, W), 80 + seed)
        if u8.numel() >= 256:
            assert u8.unique().numel() == 256
        if form == "u8":
            got = (crop_d4_u8(u8.to(dev), items_d, S),)
            want = (O.crop_d4(u8.numpy(), items, S),)
            assert got[0].dtype == torch.uint8
        else:
            labels = torch.tensor([7, -3, 2 ** 40 + 5], dtype=torch.int64)
            got = crop_d4_u8_f32(u8.to(dev), labels.to(dev), items_d, S)
            want = O.crop_d4_u8_f32(u8.numpy(), labels.numpy(), items, S)
            assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64
            # the same quotient with torch on the host (ToTensor's `.div(255)`)
            assert torch.equal(torch.from_numpy(want[0]), torch.from_numpy(O.crop_d4(u8.numpy(), items, S)).float().div(255))
    return tuple(g.cpu() for g in got), tuple(torch.from_numpy(np.ascontiguousarray(w)) for w in want)


# ---------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_crop_d4_bit_exact(dev, shape, form):
    c, H, W, S = shape
    items = _items(H, W, S)
    assert len(items) == 24 and all(O.is_valid(it, L, H, W, S) for it in items)
    got, want = _run(form, dev, shape, items)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = (g != w).flatten(1).any(dim=1).nonzero().flatten().tolist() if g.dim() > 1 else (g != w).nonzero().flatten().tolist()
        assert torch.equal(g, w), (form, shape, k, "items", [items[i].tolist() for i in bad])
    if form == "pairs":
        assert float(got[0].min()) < 0 and float(got[0].max()) > 1  # values outside [-1, 1] pass through unclipped


@pytest.mark.parametrize("form", FORMS)
def test_one_item(dev, form):
    for code, shape in ((5, SHAPES[2]), (2, SHAPES[0])):
        c, H, W, S = shape
        items = np.array([[1, H - S, 1, code]], dtype=np.int32)
        got, want = _run(form, dev, shape, items, seed=1)
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (form, shape)


@pytest.mark.parametrize("form", FORMS)
def test_invalid_items_and_untouched_guards(dev, form):
    """Items that are out of range in every way, between valid ones: zeros (label -1) for them, the right windows for the rest,
    and not a byte written outside the n output rows (sentinel-filled buffers with a guard row on each side)."""
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    c, H, W, S = 2, 40, 72, 33
    items = np.array([[1, 3, 5, 6], [L, 0, 0, 0], [0, H - S, W - S, 3], [-1, 0, 0, 0], [2, H - S + 1, 0, 0], [2, 0, -1, 1],
                      [1, 0, 0, 8], [1, 0, 0, -1], [2, 1, 2, 7], [0, -1, 0, 4], [0, 0, W - S + 1, 5], [2, 7, 39, 4]], dtype=np.int32)
    ok = [O.is_valid(it, L, H, W, S) for it in items]
    assert ok == [True, False, True, False, False, False, False, False, True, False, False, True]
    n = len(items)
    items_d = torch.from_numpy(items).to(dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def guarded(bands, dtype, sentinel):
        return torch.full((n + 2, bands, S, S), sentinel, dtype=dtype, device=dev)

    if form == "pairs":
        sar, ndvi = _f32_cache((2, H, W), 90), _f32_cache((1, H, W), 91)
        sar_d, ndvi_d = sar.to(dev), ndvi.to(dev)
        outs = [guarded(2, torch.float32, -7.0), guarded(1, torch.float32, -7.0)]
        st = lib.drs_crop_d4_pairs_f32(ptr(sar_d), ptr(ndvi_d), ptr(items_d), n, L, 2, 1, H, W, S, ptr(outs[0][1]), ptr(outs[1][1]),
                                       stream)
        want = O.crop_d4_pairs(sar.numpy(), ndvi.numpy(), items, S)
        sentinels = [-7.0, -7.0]
    else:
        u8 = _u8_cache((c, H, W), 92)
        u8_d = u8.to(dev)
        if form == "u8":
            outs = [guarded(c, torch.uint8, 0xA5)]
            st = lib.drs_crop_d4_u8(ptr(u8_d), ptr(items_d), n, L, c, H, W, S, ptr(outs[0][1]), stream)
            want = (O.crop_d4(u8.numpy(), items, S),)
            sentinels = [0xA5]
        else:
            labels = torch.tensor([11, 12, 13], dtype=torch.int64)
            labels_d = labels.to(dev)
            outs = [guarded(c, torch.float32, -7.0), torch.full((n + 2,), -99, dtype=torch.int64, device=dev)]
            st = lib.drs_crop_d4_u8_f32(ptr(u8_d), ptr(labels_d), ptr(items_d), n, L, c, H, W, S, ptr(outs[0][1]), ptr(outs[1][1:]),
                                        stream)
            want = O.crop_d4_u8_f32(u8.numpy(), labels.numpy(), items, S)
            assert want[1].tolist() == [12, -1, 11, -1, -1, -1, -1, -1, 13, -1, -1, 13]
            sentinels = [-7.0, -99]
    assert st == 0, lib.drs_last_error()
    torch.cuda.synchronize(dev)
    for out, w, sentinel in zip(outs, want, sentinels):
        out = out.cpu()
        w = torch.from_numpy(np.ascontiguousarray(w))
        assert bool((out[0] == sentinel).all()) and bool((out[-1] == sentinel).all()), form
        assert torch.equal(out[1:-1], w), form
        if out.dim() == 4:
            assert not out[1:-1][~torch.tensor(ok)].any() and out[1:-1][torch.tensor(ok)].flatten(1).any(dim=1).all(), form


@pytest.mark.parametrize("form", ["u8", "u8_f32"])
def test_windows_past_two_gib(dev, form):
    """Cache offsets beyond 2^31 bytes: the bottom-right 64 x 64 window of the last image of a cache of 2049 images of 2^20
    bytes, under a transposing code - its last load ends on the allocation's last byte - and the top-left window of image 0.
    The cache is allocated, not filled: only the windows that are read are written."""
    from diffusionremotesensing_amd.augment import crop_d4_u8, crop_d4_u8_f32
    big, S = 2049, 64
    gen = torch.Generator().manual_seed(50)
    win = torch.randint(0, 256, (2, 1, S, S), generator=gen, dtype=torch.uint8)
    u8 = torch.empty((big, 1, 1024, 1024), dtype=torch.uint8, device=dev)
    u8[big - 1, :, 1024 - S:, 1024 - S:] = win[0].to(dev)
    u8[0, :, :S, :S] = win[1].to(dev)
    items = np.array([[big - 1, 1024 - S, 1024 - S, 5], [0, 0, 0, 0], [big - 1, 1024 - S, 1024 - S, 3]], dtype=np.int32)
    want = torch.from_numpy(np.stack([O.d4(win[0].numpy(), 5), win[1].numpy(), O.d4(win[0].numpy(), 3)]))
    items_d = torch.from_numpy(items).to(dev)
    if form == "u8":
        assert torch.equal(crop_d4_u8(u8, items_d, S).cpu(), want)
    else:
        labels = torch.arange(big, dtype=torch.int64, device=dev)
        img, lab = crop_d4_u8_f32(u8, labels, items_d, S)
        assert torch.equal(img.cpu(), want.float().div(255)) and lab.cpu().tolist() == [big - 1, 0, big - 1]
    del u8
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# feeds
# ---------------------------------------------------------------------------------------------
def _centre(cache, size):
    H, W = cache.shape[2:]
    y0, x0 = (H - size) // 2, (W - size) // 2
    return cache[:, :, y0:y0 + size, x0:x0 + size].contiguous()


def test_superres_feed_crops_then_degrades(dev):
    from diffusionremotesensing_amd.degradation import DeviceSuperresFeed, downblur
    cache = _u8_cache((3, 24, 24), 100, length=4)
    feed = DeviceSuperresFeed(cache.to(dev), 2, 0.5, batch_size=3, shuffle=False, crop_size=16, augment="d4")
    seen, codes = [], set()
    for x, y in feed:
        items = feed.last_items
        assert items.dtype == np.int32 and items.shape == (x.shape[0], 4) and all(O.is_valid(it, 4, 24, 24, 16) for it in items)
        crop = torch.from_numpy(O.crop_d4(cache.numpy(), items, 16))
        assert y.shape[1:] == (3, 16, 16) and x.shape[1:] == (3, 8, 8)
        assert torch.equal(y.cpu(), crop.float() / 255)
        want_x, want_y = downblur(crop.to(dev), 2, feed.blur_radius)  # the degradation saw exactly those bytes
        assert torch.equal(x, want_x) and torch.equal(y, want_y)
        seen += items[:, 0].tolist()
        codes |= set(items[:, 3].tolist())
    assert seen == [0, 1, 2, 3] and len(feed) == 2
    x, y = feed.item(2)  # the centre window, no symmetry
    assert torch.equal(y.cpu(), _centre(cache, 16)[2].float() / 255)


def test_superres_fixed_crop_is_the_feed_over_the_centre_crops(dev):
    from diffusionremotesensing_amd.degradation import DeviceSuperresFeed
    cache = _u8_cache((3, 24, 24), 101, length=4)
    a = DeviceSuperresFeed(cache.to(dev), 2, 0.75, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(5),
                           crop_size=16, augment="d4", num_crops=3, fixed_crop=True)
    b = DeviceSuperresFeed(_centre(cache, 16).to(dev), 2, 0.75, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(5))
    assert len(a) == len(b) == 2
    for _ in range(2):  # two epochs: the ordering generators move alike
        got, want = list(a), list(b)
        assert len(got) == len(want) == 2
        for (x, y), (wx, wy) in zip(got, want):
            assert torch.equal(x, wx) and torch.equal(y, wy)
    assert a.last_items[:, 1:].tolist() == [[4, 4, 0]] * len(a.last_items)


@pytest.mark.parametrize("kind", ["plus", "soft"])
def test_bsr_fixed_crop_is_the_feed_over_the_centre_crops(dev, kind):
    from diffusionremotesensing_amd.bsr import DeviceBSRFeed
    cache = _u8_cache((3, 24, 24), 102, length=4)
    a = DeviceBSRFeed(cache.to(dev), 2, batch_size=3, kind=kind, seed=7, fixed=True, crop_size=16, fixed_crop=True)
    b = DeviceBSRFeed(_centre(cache, 16).to(dev), 2, batch_size=3, kind=kind, seed=7, fixed=True)
    got, want = list(a), list(b)
    assert len(got) == len(want) == len(a) == 2
    for (x, y), (wx, wy) in zip(got, want):
        assert x.shape[1:] == (3, 8, 8) and y.shape[1:] == (3, 16, 16)
        assert torch.equal(x, wx) and torch.equal(y, wy)
    x, y = a.item(1)
    wx, wy = b.item(1)
    assert torch.equal(x, wx) and torch.equal(y, wy)


def test_bsr_feed_active(dev):
    """An augmenting BSRGAN feed: the recipe is drawn for the window, and the item generator is not the recipe generator - the
    same seed gives the recipes of the plain feed over windows of that size."""
    from diffusionremotesensing_amd.bsr import DeviceBSRFeed
    cache = _u8_cache((3, 24, 24), 103, length=4)
    feed = DeviceBSRFeed(cache.to(dev), 2, batch_size=4, shuffle=False, kind="soft", seed=3, crop_size=16, augment="d4", augment_seed=9)
    (x, y), = list(feed)
    assert x.shape == (4, 3, 8, 8) and y.shape == (4, 3, 16, 16)
    assert np.array_equal(feed.last_items, O.draw_items(np.random.default_rng([9, 0]), np.arange(4), 24, 24, 16, "d4"))
    crop = torch.from_numpy(O.crop_d4(cache.numpy(), feed.last_items, 16))
    assert torch.equal(y.cpu(), crop.float().div(255))  # kind "soft" does not sharpen: HR is the window
    plain = DeviceBSRFeed(crop.to(dev), 2, batch_size=4, shuffle=False, kind="soft", seed=3)
    (wx, wy), = list(plain)
    assert torch.equal(x, wx) and torch.equal(y, wy)


def test_sar_and_class_feeds_active(dev):
    from diffusionremotesensing_amd.feeds import DeviceClassFeed, DeviceSarNdviFeed
    sar, ndvi = _f32_cache((2, 20, 20), 110, length=5), _f32_cache((1, 20, 20), 111, length=5)
    feed = DeviceSarNdviFeed(sar.to(dev), ndvi.to(dev), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(2),
                             crop_size=12, augment="d4", num_crops=2, augment_seed=4)
    assert len(feed) == 3
    src = []
    for x, y in feed:
        items = feed.last_items
        want_x, want_y = O.crop_d4_pairs(sar.numpy(), ndvi.numpy(), items, 12)  # one window and one code for the pair
        assert torch.equal(x.cpu(), torch.from_numpy(want_x)) and torch.equal(y.cpu(), torch.from_numpy(want_y))
        src += items[:, 0].tolist()
    gen = torch.Generator().manual_seed(2)
    assert src == torch.cat([torch.randperm(5, generator=gen), torch.randperm(5, generator=gen)]).tolist()
    x, y = feed.item(3)
    assert torch.equal(x.cpu(), (_centre(sar, 12)[3] + 1) / 2) and torch.equal(y.cpu(), (_centre(ndvi, 12)[3] + 1) / 2)

    u8 = _u8_cache((3, 20, 20), 112, length=5)
    labels = torch.tensor([4, 0, 2, 2, 1], dtype=torch.int64)
    cls = DeviceClassFeed(u8.to(dev), labels.to(dev), ["a", "b", "c", "d", "e"], batch_size=4, shuffle=False, crop_size=12,
                          augment="d4", augment_seed=4)
    src = []
    for img, lab in cls:
        items = cls.last_items
        want_img, want_lab = O.crop_d4_u8_f32(u8.numpy(), labels.numpy(), items, 12)
        assert torch.equal(img.cpu(), torch.from_numpy(want_img)) and torch.equal(lab.cpu(), torch.from_numpy(want_lab))
        assert torch.equal(lab.cpu(), labels[torch.from_numpy(items[:, 0].astype(np.int64))])  # labels follow src
        src += items[:, 0].tolist()
    assert src == [0, 1, 2, 3, 4]
    img, label = cls.dataset[4]
    assert torch.equal(img.cpu(), _centre(u8, 12)[4].float().div(255)) and label == 1 and isinstance(label, int)


def test_item_streams_of_feeds(dev):
    from diffusionremotesensing_amd.feeds import DeviceSarNdviFeed
    sar, ndvi = _f32_cache((2, 20, 20), 120, length=6).to(dev), _f32_cache((1, 20, 20), 121, length=6).to(dev)

    def epoch(feed):
        rows = []
        for _ in feed:
            rows.append(feed.last_items.copy())
        return np.concatenate(rows)

    def make(**kw):
        return DeviceSarNdviFeed(sar, ndvi, batch_size=4, shuffle=False, crop_size=8, augment="d4", **kw)
    a, b, other_rank = make(augment_seed=1), make(augment_seed=1), make(augment_seed=1, augment_rank=1)
    first = epoch(a)
    assert np.array_equal(first, epoch(b))
    assert not np.array_equal(first, epoch(other_rank))
    second = epoch(a)
    assert np.array_equal(first[:, 0], second[:, 0]) and not np.array_equal(first, second)  # a new epoch: new windows


def test_default_feeds_are_todays(dev):
    """With today's arguments each feed yields what the existing wrappers give for the same index vectors - same launches, same
    draws from its generator - and carries no items."""
    from diffusionremotesensing_amd.bsr import DeviceBSRFeed, degrade, draw_recipe
    from diffusionremotesensing_amd.degradation import DeviceSuperresFeed, downblur
    from diffusionremotesensing_amd.feeds import DeviceClassFeed, DeviceSarNdviFeed, gather_pairs, gather_u8
    u8 = _u8_cache((3, 16, 16), 130, length=5).to(dev)
    order = torch.randperm(5, generator=torch.Generator().manual_seed(8)).to(dev)
    sup = DeviceSuperresFeed(u8, 2, 0.5, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(8))
    for k, (x, y) in enumerate(sup):
        wx, wy = downblur(u8[order[4 * k:4 * k + 4]], 2, 0.5)
        assert torch.equal(x, wx) and torch.equal(y, wy)
    sar, ndvi = _f32_cache((2, 16, 16), 131, length=5).to(dev), _f32_cache((1, 16, 16), 132, length=5).to(dev)
    pairs = DeviceSarNdviFeed(sar, ndvi, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(8))
    for k, (x, y) in enumerate(pairs):
        wx, wy = gather_pairs(sar, ndvi, order[4 * k:4 * k + 4])
        assert torch.equal(x, wx) and torch.equal(y, wy)
    labels = torch.arange(5, dtype=torch.int64, device=dev)
    cls = DeviceClassFeed(u8, labels, ["a"], batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(8))
    for k, (img, lab) in enumerate(cls):
        wi, wl = gather_u8(u8, labels, order[4 * k:4 * k + 4])
        assert torch.equal(img, wi) and torch.equal(lab, wl)
    bsr = DeviceBSRFeed(u8, 2, batch_size=4, shuffle=True, kind="soft", seed=6)
    rng, gen = np.random.default_rng(6), torch.Generator(device=dev).manual_seed(6)
    perm = torch.from_numpy(rng.permutation(5)).to(dev)
    for k, (x, y) in enumerate(bsr):
        hr = gather_u8(u8, torch.zeros(5, dtype=torch.int64, device=dev), perm[4 * k:4 * k + 4])[0]
        wx, wy = degrade(hr, draw_recipe(rng, hr.shape[0], 3, 16, 16, 2, "soft"), generator=gen)
        assert torch.equal(x, wx) and torch.equal(y, wy)
    for feed in (sup, pairs, cls, bsr):
        assert feed.last_items is None and feed._aug is None and len(feed) == 2


# ---------------------------------------------------------------------------------------------
# end to end, at the smallest shape the network takes
# ---------------------------------------------------------------------------------------------
_RUN = ["--image_size", "16", "--noise_steps", "10", "--epochs", "1", "--batch_size", "2", "--check_preds_epoch", "1",
        "--loss", "MSE"]


def test_sar_trainer_on_windows_of_scenes(dev, tmp_path, monkeypatch, capsys):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    data = str(tmp_path / "data")
    write_sar_folder(os.path.join(data, "train"), ["d", "b", "a", "c"], 24, seed=1)
    write_sar_folder(os.path.join(data, "test"), ["y", "x"], 24, seed=2)
    monkeypatch.chdir(tmp_path)
    steps, inner = [], S.Diffusion.train_step

    def counted(self, *args, **kwargs):
        steps.append(tuple(args[3].shape))  # (model, optimizer, loss_function, SAR batch, ...)
        return inner(self, *args, **kwargs)
    monkeypatch.setattr(S.Diffusion, "train_step", counted)
    torch.manual_seed(0)
    S.main(_RUN + ["--model_name", "sar_scenes", "--dataset_path", data, "--scene_size", "24", "--augment", "d4", "--num_crops", "2"])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Training snapshot saved" in out
    assert os.path.exists(tmp_path / "models_run" / "sar_scenes" / "weights" / "snapshot.pt")
    res = torch.load(tmp_path / "models_run" / "sar_scenes" / "results" / "SAR_TO_NDVI_results.pt")
    assert tuple(res.shape) == (4, 1, 16, 16) and bool(torch.isfinite(res).all())
    assert len(steps) == math.ceil(2 * 4 / 2) and all(s == (2, 2, 16, 16) for s in steps)
    with pytest.raises(ValueError, match="24 x 24, --scene_size is 32"):
        S.main(_RUN + ["--model_name", "sar_scenes32", "--dataset_path", data, "--scene_size", "32"])


def test_superres_trainer_on_windows_of_scenes(dev, tmp_path, monkeypatch, capsys):
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    T.main(_RUN + ["--model_name", "sr_scenes", "--dataset_path", "synthetic_u8:4", "--scene_size", "32", "--magnification_factor",
                   "2", "--augment", "flip", "--Blur_radius", "0.5"])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Training snapshot saved" in out
    assert os.path.exists(tmp_path / "models_run" / "sr_scenes" / "weights" / "snapshot.pt")
    res = torch.load(tmp_path / "models_run" / "sr_scenes" / "results" / "superres_results.pt")
    assert tuple(res.shape) == (4, 3, 16, 16) and bool(torch.isfinite(res).all())
