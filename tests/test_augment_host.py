"""Host side of the crop / dihedral augmentation of the device feeds (diffusionremotesensing_amd/augment.py, DESIGN.md section
20): the numpy oracle (tests/augment_oracle.py) against independent statements of the eight symmetries, the item draws, the
argument checks of the three C entry points, the command lines and the epoch arithmetic of active feeds.  No GPU."""
import itertools

import numpy as np
import pytest
import torch

import augment_oracle as O


def _image(c=2, s=5):
    """(c, s, s) with all pixels different."""
    return np.arange(c * s * s, dtype=np.int64).reshape(c, s, s)


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def test_oracle_codes_against_flip_and_rot90():
    w = _image()
    assert np.array_equal(O.d4(w, 0), w)
    assert np.array_equal(O.d4(w, 1), np.flip(w, axis=-1))
    assert np.array_equal(O.d4(w, 2), np.flip(w, axis=-2))
    assert np.array_equal(O.d4(w, 3), np.flip(w, axis=(-2, -1)))
    assert np.array_equal(O.d4(w, 3), np.rot90(w, 2, axes=(-2, -1)))
    assert np.array_equal(O.d4(w, 4), np.swapaxes(w, -1, -2))
    assert np.array_equal(O.d4(w, 6), np.rot90(w, 1, axes=(-2, -1)))   # a quarter turn counter-clockwise
    assert np.array_equal(O.d4(w, 5), np.rot90(w, -1, axes=(-2, -1)))  # a quarter turn clockwise
    assert np.array_equal(O.d4(w, 7), np.flip(np.swapaxes(w, -1, -2), axis=(-2, -1)))  # the anti-transpose


def test_oracle_element_form():
    """out[c, y, x] = w[c, y', x'] with (u, v) = (code & 2 ? S-1-y : y, code & 1 ? S-1-x : x), (y', x') = code & 4 ? (v, u) : (u, v)."""
    w, s = _image(), 5
    for code in range(8):
        got = O.d4(w, code)
        for y, x in itertools.product(range(s), range(s)):
            u, v = (s - 1 - y if code & 2 else y), (s - 1 - x if code & 1 else x)
            yy, xx = (v, u) if code & 4 else (u, v)
            assert np.array_equal(got[:, y, x], w[:, yy, xx]), (code, y, x)


def test_oracle_codes_form_a_group():
    w = _image()
    eight = [np.ascontiguousarray(O.d4(w, code)) for code in range(8)]
    for a, b in itertools.combinations(range(8), 2):
        assert not np.array_equal(eight[a], eight[b]), (a, b)
    for a, b in itertools.product(range(8), range(8)):
        both = O.d4(O.d4(w, a), b)
        assert sum(np.array_equal(both, e) for e in eight) == 1, (a, b)


def test_oracle_windows_and_invalid_items():
    cache = np.arange(3 * 2 * 6 * 7, dtype=np.uint8).reshape(3, 2, 6, 7)
    items = np.array([[2, 1, 2, 0], [0, 2, 3, 5], [3, 0, 0, 0], [-1, 0, 0, 0], [1, 3, 0, 0], [1, 0, 4, 0], [1, -1, 0, 0],
                      [1, 0, 0, 8], [1, 0, 0, -1], [1, 2, 3, 7]], dtype=np.int32)
    out = O.crop_d4(cache, items, 4)
    assert out.dtype == np.uint8 and out.shape == (10, 2, 4, 4)
    assert np.array_equal(out[0], cache[2, :, 1:5, 2:6])
    assert np.array_equal(out[1], np.rot90(cache[0, :, 2:6, 3:7], -1, axes=(-2, -1)))
    assert np.array_equal(out[9], np.flip(np.swapaxes(cache[1, :, 2:6, 3:7], -1, -2), axis=(-2, -1)))
    assert not out[2:9].any()
    img, lab = O.crop_d4_u8_f32(cache, np.array([10, 11, 12]), items, 4)
    assert img.dtype == np.float32 and lab.tolist() == [12, 10, -1, -1, -1, -1, -1, -1, -1, 11]
    assert np.array_equal(img, out.astype(np.float32) / np.float32(255))
    f = (cache.astype(np.float32) - 100) / 64
    a, b = O.crop_d4_pairs(f, f[:, :1], items, 4)
    assert np.array_equal(a[0], (f[2, :, 1:5, 2:6] + 1) / 2) and np.array_equal(b[0], a[0][:1]) and not a[2:9].any() and not b[2:9].any()


# ---------------------------------------------------------------------------------------------
# draw_items / centre_items
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,codes", [("none", {0}), ("flip", {0, 1, 2, 3}), ("d4", set(range(8)))])
def test_draw_items(mode, codes):
    from diffusionremotesensing_amd.augment import draw_items
    n, H, W, S = 4096, 12, 20, 8
    src = np.arange(n) % 7
    items = draw_items(np.random.default_rng(11), src, H, W, S, mode)
    assert items.dtype == np.int32 and items.shape == (n, 4) and np.array_equal(items[:, 0], src)
    assert set(items[:, 3].tolist()) == codes
    if mode == "flip":
        assert not (items[:, 3] & 4).any()
    assert items[:, 1].min() == 0 and items[:, 1].max() == H - S and items[:, 2].min() == 0 and items[:, 2].max() == W - S
    assert all(O.is_valid(it, 7, H, W, S) for it in items)
    # the draw order: codes, then row offsets, then column offsets, n values each
    rng = np.random.default_rng(11)
    code = rng.integers(0, len(codes), n)
    y0 = rng.integers(0, H - S + 1, n)
    x0 = rng.integers(0, W - S + 1, n)
    assert np.array_equal(items[:, 3], code) and np.array_equal(items[:, 1], y0) and np.array_equal(items[:, 2], x0)
    assert np.array_equal(items, O.draw_items(np.random.default_rng(11), src, H, W, S, mode))


def test_draw_items_edges():
    from diffusionremotesensing_amd.augment import centre_items, draw_items
    items = draw_items(np.random.default_rng(0), [3, 1], 8, 8, 8, "d4")  # H - S = 0
    assert items[:, 1:3].tolist() == [[0, 0], [0, 0]] and items[:, 0].tolist() == [3, 1]
    with pytest.raises(ValueError, match="must be one of"):
        draw_items(np.random.default_rng(0), [0], 8, 8, 4, "rot")
    with pytest.raises(ValueError, match="does not fit"):
        draw_items(np.random.default_rng(0), [0], 8, 6, 7, "none")
    c = centre_items([4, 0, 4], 9, 12, 4)
    assert c.dtype == np.int32 and c.tolist() == [[4, 2, 4, 0], [0, 2, 4, 0], [4, 2, 4, 0]]
    assert np.array_equal(c, O.centre_items([4, 0, 4], 9, 12, 4))
    with pytest.raises(ValueError, match="does not fit"):
        centre_items([0], 4, 4, 5)


# ---------------------------------------------------------------------------------------------
# C entry points
# ---------------------------------------------------------------------------------------------
def test_entry_points_validate_without_gpu():
    import ctypes as C
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    assert lib.drs_abi_version() == 8
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    calls = {
        "crop_d4_u8": lambda q, n, L, c, H, W, S: lib.drs_crop_d4_u8(q, q, n, L, c, H, W, S, q, None),
        "crop_d4_u8_f32": lambda q, n, L, c, H, W, S: lib.drs_crop_d4_u8_f32(q, q, q, n, L, c, H, W, S, q, q, None),
        "crop_d4_pairs_f32": lambda q, n, L, c, H, W, S: lib.drs_crop_d4_pairs_f32(q, q, q, n, L, c, 1, H, W, S, q, q, None),
    }
    for name, call in calls.items():
        assert call(None, 1, 1, 1, 4, 4, 4) == 1
        assert b"null pointer" in lib.drs_last_error() and name.encode() in lib.drs_last_error()
        #            n  L  C  H  W  S
        for bad in ((0, 1, 1, 4, 4, 4), (-1, 1, 1, 4, 4, 4), (1, 1, 1, 4, 4, 0), (1, 1, 1, 4, 4, -2), (1, 1, 1, 4, 8, 5),
                    (1, 1, 1, 8, 4, 5), (1, 0, 1, 4, 4, 4), (1, 1, 0, 4, 4, 4)):
            assert call(p, *bad) == 2, (name, bad)
            assert name.encode() in lib.drs_last_error(), (name, bad)
    assert lib.drs_crop_d4_u8(p, None, 1, 1, 1, 4, 4, 4, p, None) == 1
    assert lib.drs_crop_d4_u8_f32(p, None, p, 1, 1, 1, 4, 4, 4, p, p, None) == 1
    assert lib.drs_crop_d4_pairs_f32(p, p, p, 1, 1, 2, 0, 4, 4, 4, p, p, None) == 2  # no NDVI band


def test_wrappers_refuse_host_tensors_and_bad_items():
    from diffusionremotesensing_amd.augment import crop_d4_pairs, crop_d4_u8, crop_d4_u8_f32
    items = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm device"):
        crop_d4_u8(torch.zeros((1, 1, 4, 4), dtype=torch.uint8), items, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        crop_d4_u8_f32(torch.zeros((1, 1, 4, 4), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), items, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        crop_d4_pairs(torch.zeros((1, 1, 4, 4)), torch.zeros((1, 1, 4, 4)), items, 4)
    with pytest.raises(RuntimeError, match="uint8"):
        crop_d4_u8(torch.zeros((1, 1, 4, 4)), items, 4)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def test_add_augment_args():
    import argparse
    from diffusionremotesensing_amd.augment import add_augment_args, feed_kwargs, scene_size
    p = add_augment_args(argparse.ArgumentParser())
    a = p.parse_args([])
    assert (a.scene_size, a.augment, a.augment_seed, a.num_crops) == (None, "none", 0, 1)
    a = p.parse_args(["--scene_size", "64", "--augment", "d4", "--augment_seed", "9", "--num_crops", "3"])
    assert (a.scene_size, a.augment, a.augment_seed, a.num_crops) == (64, "d4", 9, 3)
    with pytest.raises(SystemExit):
        p.parse_args(["--augment", "rot45"])
    # a parser that has --num_crops already keeps its one action; the help text says what the flag does now
    q = argparse.ArgumentParser()
    q.add_argument("--num_crops", type=int, default=1, help="old")
    add_augment_args(q)
    crops = [x for x in q._actions if x.dest == "num_crops"]
    assert len(crops) == 1 and "no effect unless --scene_size or --augment" in crops[0].help
    # what the feed builders make of the flags
    a.image_size = 32
    assert scene_size(a) == 64
    assert feed_kwargs(a, rank=2) == {"crop_size": 32, "augment": "d4", "num_crops": 3, "augment_seed": 9, "augment_rank": 2}
    assert feed_kwargs(a, rank=2, fixed=True) == {"crop_size": 32, "fixed_crop": True}
    a.scene_size = 16
    with pytest.raises(ValueError, match="--scene_size 16 is smaller than --image_size 32"):
        scene_size(a)
    plain = argparse.Namespace(image_size=32)  # a command line without the flags: the feeds are what they were
    assert scene_size(plain) == 32 and feed_kwargs(plain) == {} and feed_kwargs(plain, fixed=True) == {}
    only_aug = argparse.Namespace(image_size=32, augment="flip", num_crops=2)
    assert feed_kwargs(only_aug)["crop_size"] is None and feed_kwargs(only_aug, fixed=True) == {}


def test_trainer_parsers_take_the_flags(monkeypatch):
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    from diffusionremotesensing_amd import train_diffusion_superres as T
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as G
    flags = ["--scene_size", "48", "--augment", "flip", "--augment_seed", "3", "--num_crops", "2"]
    for name, mod in (("superres", T), ("sar", S), ("generation", G)):
        seen = {}
        monkeypatch.setattr(mod, "launch", lambda args, seen=seen: seen.update(vars(args)))
        mod.main(["--model_name", "m", "--image_size", "16"] + flags)
        assert (seen["scene_size"], seen["augment"], seen["augment_seed"], seen["num_crops"]) == (48, "flip", 3, 2), name
        seen.clear()
        mod.main(["--model_name", "m", "--image_size", "16"])
        assert (seen["scene_size"], seen["augment"], seen["augment_seed"], seen["num_crops"]) == (None, "none", 0, 1), name
    # the parsers other tests pin keep their flag sets
    for p in (T.build_arg_parser(), S.build_arg_parser(), S.train_arg_parser(), G.build_arg_parser(), evaluate.evaluate_arg_parser()):
        assert not {"scene_size", "augment", "augment_seed"} & {a.dest for a in p._actions}
    helps = {a.dest: a.help for a in T.build_arg_parser()._actions}
    assert "unused" not in helps["num_crops"]


def test_launchers_check_scene_size_before_any_device(tmp_path):
    import argparse
    from feeds_fixtures import write_sar_folder
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    write_sar_folder(str(tmp_path / "d" / "train"), ["a", "b"], 8)
    args = S.train_main_parser().parse_args(["--model_name", "s", "--image_size", "4", "--scene_size", "16",
                                             "--dataset_path", str(tmp_path / "d")])
    with pytest.raises(ValueError, match="8 x 8, --scene_size is 16"):
        S.folder_feed(args, "cpu", "train")
    args.scene_size = 2
    with pytest.raises(ValueError, match="--scene_size 2 is smaller than --image_size 4"):
        S.folder_feed(args, "cpu", "train")
    args.scene_size = 8
    train = S.folder_feed(args, "cpu", "train")
    assert train._aug is not None and train._aug.size == 4 and not train._aug.fixed
    assert S.folder_feed(args, "cpu", "train", limit=1)._aug.fixed  # the final sampling's items: centre windows
    assert isinstance(args, argparse.Namespace)


# ---------------------------------------------------------------------------------------------
# epoch arithmetic (the constructors take host tensors; making a batch needs the device)
# ---------------------------------------------------------------------------------------------
def _feeds(**kw):
    from diffusionremotesensing_amd.degradation import DeviceSuperresFeed
    from diffusionremotesensing_amd.feeds import DeviceClassFeed, DeviceSarNdviFeed
    u8 = torch.zeros((5, 3, 8, 8), dtype=torch.uint8)
    return [DeviceSuperresFeed(u8, 2, 0.5, batch_size=4, generator=torch.Generator().manual_seed(1), **kw),
            DeviceSarNdviFeed(torch.zeros((5, 2, 8, 8)), torch.zeros((5, 1, 8, 8)), batch_size=4,
                              generator=torch.Generator().manual_seed(1), **kw),
            DeviceClassFeed(u8, torch.arange(5), ["a"], batch_size=4, generator=torch.Generator().manual_seed(1), **kw)]


def test_epoch_is_num_crops_passes():
    for feed in _feeds(crop_size=4, augment="d4", num_crops=3):
        assert len(feed) == 4
        src = feed.epoch_order()
        assert src.dtype == torch.int64 and sorted(src.tolist()) == sorted(list(range(5)) * 3)
        # each pass is one order of the feed's generator, drawn as a pass is drawn today
        gen = torch.Generator().manual_seed(1)
        assert torch.equal(src, torch.cat([torch.randperm(5, generator=gen) for _ in range(3)]))
        assert feed.last_items is None
    for feed in _feeds(crop_size=4, augment="d4", num_crops=3, fixed_crop=True):
        assert len(feed) == 2 and sorted(feed.epoch_order().tolist()) == list(range(5))
        assert feed._aug.items([3, 1]).tolist() == [[3, 2, 2, 0], [1, 2, 2, 0]]
    for feed in _feeds():  # today's arguments: nothing new is attached
        assert len(feed) == 2 and feed._aug is None and feed.last_items is None
    for feed in _feeds(augment="flip"):  # an augment alone: windows of the cache's own size
        assert len(feed) == 2 and feed._aug.size == 8


def test_feed_argument_errors():
    from diffusionremotesensing_amd.feeds import DeviceSarNdviFeed
    sar, ndvi = torch.zeros((2, 2, 8, 6)), torch.zeros((2, 1, 8, 6))
    assert DeviceSarNdviFeed(sar, ndvi, crop_size=6)._aug.size == 6  # H != W is fine with a window
    with pytest.raises(ValueError, match="square"):
        DeviceSarNdviFeed(sar, ndvi, augment="d4")
    with pytest.raises(ValueError, match="does not fit"):
        DeviceSarNdviFeed(sar, ndvi, crop_size=7)
    with pytest.raises(ValueError, match="must be one of"):
        DeviceSarNdviFeed(sar, ndvi, crop_size=4, augment="rot")
    with pytest.raises(ValueError, match="num_crops"):
        DeviceSarNdviFeed(sar, ndvi, crop_size=4, num_crops=0)


def test_item_streams_by_seed_and_rank():
    from diffusionremotesensing_amd.augment import FeedAugment
    src = np.arange(64) % 5
    a, b = FeedAugment(8, 8, 4, "d4", augment_seed=3), FeedAugment(8, 8, 4, "d4", augment_seed=3)
    other_rank, other_seed = FeedAugment(8, 8, 4, "d4", augment_seed=3, augment_rank=1), FeedAugment(8, 8, 4, "d4", augment_seed=4)
    first = a.items(src)
    assert np.array_equal(first, b.items(src))
    assert np.array_equal(first, O.draw_items(np.random.default_rng([3, 0]), src, 8, 8, 4, "d4"))
    assert not np.array_equal(first, other_rank.items(src)) and not np.array_equal(first, other_seed.items(src))
    assert not np.array_equal(first, a.items(src))  # the generator moves on
