"""Host side of the SAR -> NDVI and class-folder data feeds (diffusionremotesensing_amd/feeds.py): the folder readers against
the reference dataset's own items (tests/golden/feeds, tools/make_golden_feeds.py) and against Pillow, their error cases and
sharding, the argument checks of the two C entry points, and the command lines.  No GPU."""
import os
import shutil

import numpy as np
import pytest
import torch

from feeds_fixtures import GOLDEN_FEEDS, golden_items, pillow_bytes, write_class_tree, write_sar_folder


# ---------------------------------------------------------------------------------------------
# load_sar_ndvi_folder
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,data_format", [("pt", "torch"), ("npy", "numpy")])
def test_sar_loader_gives_the_reference_items(fmt, data_format):
    from diffusionremotesensing_amd.feeds import load_sar_ndvi_folder
    items, names = golden_items()
    assert names == sorted(names) == ["a_7", "s_10", "s_2"]
    sar, ndvi = load_sar_ndvi_folder(os.path.join(GOLDEN_FEEDS, fmt, "train"), data_format)
    assert sar.dtype == ndvi.dtype == torch.float32 and tuple(sar.shape) == (3, 2, 8, 8) and tuple(ndvi.shape) == (3, 1, 8, 8)
    assert float(sar.min()) < -1 and float(sar.max()) > 1  # the raw file values: nothing clipped or rescaled on the host
    for i, (want_sar, want_ndvi) in enumerate(items):
        assert torch.equal((sar[i] + 1) / 2, want_sar) and torch.equal((ndvi[i] + 1) / 2, want_ndvi), (fmt, i)


def _copy_golden(tmp_path):
    root = str(tmp_path / "train")
    shutil.copytree(os.path.join(GOLDEN_FEEDS, "pt", "train"), root)
    return root


def test_sar_loader_errors(tmp_path):
    from diffusionremotesensing_amd.feeds import load_sar_ndvi_folder
    root = _copy_golden(tmp_path)
    with pytest.raises(ValueError, match="data_format"):
        load_sar_ndvi_folder(root, "PIL")
    os.remove(os.path.join(root, "opt", "s_10.pt"))
    with pytest.raises(ValueError, match=r"s_10\.pt.*no partner"):
        load_sar_ndvi_folder(root)
    torch.save(torch.zeros(1, 8, 9), os.path.join(root, "opt", "s_10.pt"))
    with pytest.raises(ValueError, match=r"opt.s_10\.pt.*differs"):
        load_sar_ndvi_folder(root)
    torch.save(torch.zeros(8, 8), os.path.join(root, "opt", "s_10.pt"))
    with pytest.raises(ValueError, match=r"s_10\.pt.*\(C, H, W\)"):
        load_sar_ndvi_folder(root)
    torch.save(torch.zeros(17, 8, 8), os.path.join(root, "sar", "a_7.pt"))
    with pytest.raises(ValueError, match=r"a_7\.pt.*17 bands"):
        load_sar_ndvi_folder(root)
    with pytest.raises(FileNotFoundError):
        load_sar_ndvi_folder(str(tmp_path / "nowhere"))


def test_sar_loader_shards_and_limit(capsys):
    from diffusionremotesensing_amd.feeds import load_sar_ndvi_folder
    root = os.path.join(GOLDEN_FEEDS, "pt", "train")
    whole, _ = load_sar_ndvi_folder(root)
    assert capsys.readouterr().out == ""
    r0, n0 = load_sar_ndvi_folder(root, rank=0, world_size=2)
    r1, n1 = load_sar_ndvi_folder(root, rank=1, world_size=2)
    out = capsys.readouterr().out
    assert out.count("left out") == 1 and "1 of 3" in out  # 3 files over 2 ranks: 1 + 1, reported by rank 0 only
    assert r0.shape[0] == r1.shape[0] == n0.shape[0] == n1.shape[0] == 1
    assert torch.equal(r0[0], whole[0]) and torch.equal(r1[0], whole[1])
    two, two_n = load_sar_ndvi_folder(root, rank=1, world_size=2, limit=2)  # the first files of the WHOLE list
    assert torch.equal(two, whole[:2]) and two_n.shape[0] == 2
    assert load_sar_ndvi_folder(root, limit=5)[0].shape[0] == 3
    with pytest.raises(ValueError, match="cannot be sharded"):
        load_sar_ndvi_folder(root, rank=0, world_size=4)


# ---------------------------------------------------------------------------------------------
# load_class_folder_u8
# ---------------------------------------------------------------------------------------------
def test_class_loader_follows_imagefolder(tmp_path):
    from diffusionremotesensing_amd.feeds import load_class_folder_u8
    root = str(tmp_path / "tree")
    samples = write_class_tree(root, 8)
    u8, labels, classes = load_class_folder_u8(root, 8)
    assert classes == ["a_cls", "b_cls", "c_cls"]
    assert labels.dtype == torch.int64 and labels.tolist() == [lab for _, lab in samples]
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (5, 3, 8, 8)
    for i, (rel, _) in enumerate(samples):
        assert torch.equal(u8[i], pillow_bytes(os.path.join(root, rel), 8)), rel
    assert torch.equal(u8[4, 0], u8[4, 1]) and torch.equal(u8[4, 0], u8[4, 2])  # the grey-scale image as RGB
    # every second sample per rank, the fifth left out; the classes are the whole folder's on every rank
    s1, l1, c1 = load_class_folder_u8(root, 8, rank=1, world_size=2)
    assert c1 == classes and l1.tolist() == [0, 1] and torch.equal(s1, u8[1:4:2])


def test_class_loader_errors_and_npy(tmp_path):
    from diffusionremotesensing_amd.feeds import load_class_folder_u8
    root = str(tmp_path / "tree")
    write_class_tree(root, 8)
    os.makedirs(os.path.join(root, "d_cls"))
    with open(os.path.join(root, "d_cls", "readme.txt"), "w") as f:
        f.write("no image here\n")
    with pytest.raises(FileNotFoundError, match="d_cls"):
        load_class_folder_u8(root, 8)
    with pytest.raises(FileNotFoundError):
        load_class_folder_u8(str(tmp_path / "tree" / "d_cls"), 8)  # no class folder at all
    np.save(os.path.join(root, "d_cls", "five_bands.npy"), np.random.default_rng(0).random((8, 8, 5)).astype(np.float32))
    with pytest.raises(ValueError, match="band count"):
        load_class_folder_u8(root, 8)
    # a tree of .npy samples only: the project's multispectral convention (degradation.load_npy_u8)
    ms = str(tmp_path / "ms")
    os.makedirs(os.path.join(ms, "x"))
    a = np.random.default_rng(1).random((8, 8, 5)).astype(np.float32)
    np.save(os.path.join(ms, "x", "a.npy"), a)
    u8, labels, classes = load_class_folder_u8(ms, 8)
    assert classes == ["x"] and labels.tolist() == [0] and tuple(u8.shape) == (1, 5, 8, 8)
    assert np.array_equal(u8[0].numpy(), np.moveaxis((a * 255).astype(np.uint8), -1, 0))


def test_feed_surfaces_without_a_device(tmp_path):
    """What the reference's `train` / `launch` read from a loader - `len`, `.dataset.classes`, `len(.dataset)` - needs no
    device; making a batch or an item does, and says so (there is no CPU path)."""
    from diffusionremotesensing_amd.feeds import DeviceClassFeed, DeviceSarNdviFeed, load_class_folder_u8
    root = str(tmp_path / "tree")
    write_class_tree(root, 8)
    u8, labels, classes = load_class_folder_u8(root, 8)
    feed = DeviceClassFeed(u8, labels, classes, batch_size=2, shuffle=False)
    assert len(feed) == 3 and feed.classes == classes and feed.dataset.classes == classes and len(feed.dataset) == 5
    assert feed.shuffle is False
    with pytest.raises(RuntimeError, match="ROCm device"):
        feed.dataset[0]
    with pytest.raises(RuntimeError, match="ROCm device"):
        next(iter(feed))
    with pytest.raises(IndexError):
        feed.dataset[5]
    with pytest.raises(RuntimeError, match="int64"):
        DeviceClassFeed(u8, labels[:4], classes, 2)
    sar = DeviceSarNdviFeed(torch.zeros((5, 2, 8, 8)), torch.zeros((5, 1, 8, 8)), batch_size=4)
    assert len(sar) == 2 and sar.shuffle is True
    sar.shuffle = False
    with pytest.raises(RuntimeError, match="ROCm device"):
        sar.item(0)
    with pytest.raises(RuntimeError, match="uint8"):
        DeviceClassFeed(u8.float(), labels, classes, 2)


# ---------------------------------------------------------------------------------------------
# C entry points and command lines
# ---------------------------------------------------------------------------------------------
def test_entry_points_validate_without_gpu():
    import ctypes as C
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    assert lib.drs_gather_pairs_f32(None, None, None, 1, 1, 4, 4, None, None, None) == 1
    assert b"null pointer" in lib.drs_last_error()
    assert lib.drs_gather_u8_f32(None, None, None, 1, 1, 16, None, None, None) == 1
    assert b"null pointer" in lib.drs_last_error()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    for n, L, row in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (-1, 1, 4)):
        assert lib.drs_gather_pairs_f32(p, p, p, n, L, row, 4, p, p, None) == 2
        assert b"gather_pairs" in lib.drs_last_error()
        assert lib.drs_gather_u8_f32(p, p, p, n, L, row, p, p, None) == 2
        assert b"gather_u8" in lib.drs_last_error()
    assert lib.drs_gather_pairs_f32(p, p, p, 1, 1, 4, 0, p, p, None) == 2


def test_parsers():
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    from diffusionremotesensing_amd import train_diffusion_superres as T
    p = S.train_arg_parser()  # (build_arg_parser stays the reference's flag set: tests/test_sampler_host.py)
    assert {a.dest for a in p._actions} == {a.dest for a in S.build_arg_parser()._actions} | {"data_format"}
    assert p.parse_args([]).data_format == "torch"
    assert p.parse_args(["--data_format", "numpy"]).data_format == "numpy"
    with pytest.raises(SystemExit):
        p.parse_args(["--data_format", "PIL"])
    # without an argument: the super-resolution parser, as before, plus --task
    e = evaluate.evaluate_arg_parser()
    base = {a.dest for a in T.build_arg_parser()._actions}
    assert {a.dest for a in e._actions} == base | {"n_images", "out", "task"}
    args = e.parse_args(["--magnification_factor", "2"])
    assert args.task == "superres" and args.magnification_factor == 2 and args.Degradation_type == "DownBlur"
    s = evaluate.evaluate_arg_parser("sar_to_ndvi")
    args = s.parse_args(["--task", "sar_to_ndvi", "--SAR_channels", "4", "--n_images", "2", "--data_format", "numpy"])
    assert (args.task, args.SAR_channels, args.NDVI_channels, args.n_images, args.data_format) == ("sar_to_ndvi", 4, 1, 2, "numpy")
    assert not hasattr(args, "magnification_factor")
    with pytest.raises(SystemExit):
        e.parse_args(["--task", "generation"])


def test_launchers_refuse_bad_datasets_before_any_device(tmp_path, monkeypatch):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as G
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(G, "launch_device", lambda args: pytest.fail("the device was touched"))
    with pytest.raises(ValueError, match="(?s)cifar10.*download.*folder per class"):
        G.main(["--model_name", "g", "--image_size", "16", "--loss", "MSE", "--dataset_path", "cifar10"])
    # the folder checks of the SAR launcher, on the host tensors (a fake device: nothing is moved before the checks pass)
    args = S.train_arg_parser().parse_args(["--model_name", "s", "--image_size", "16", "--dataset_path", str(tmp_path / "d")])
    with pytest.raises(FileNotFoundError, match="train/sar, train/opt, test/sar and test/opt"):
        S.folder_feed(args, "cpu", "train")
    write_sar_folder(str(tmp_path / "d" / "train"), ["a", "b"], 8)
    with pytest.raises(ValueError, match="8 x 8, --image_size is 16"):
        S.folder_feed(args, "cpu", "train")
    args.image_size, args.SAR_channels = 8, 3
    with pytest.raises(ValueError, match="2 bands, --SAR_channels is 3"):
        S.folder_feed(args, "cpu", "train")
    args.SAR_channels, args.NDVI_channels = 2, 2
    with pytest.raises(ValueError, match="1 bands, --NDVI_channels is 2"):
        S.folder_feed(args, "cpu", "train")
    with pytest.raises(FileNotFoundError, match="test"):
        S.folder_feed(args, "cpu", "test")
