"""Host side of the 16-bit radiometry (diffusionremotesensing_amd/radiometry.py; no device): the fp32
definition of normalise / quantise and its round trip, the percentile rule, the uint16 loader, the command lines and the
DATA_RANGE of snapshots and train_state.pt.  tests/radiometry_oracle.py is the restatement the package's host forms (and, in
tests/test_gpu_radiometry.py, the kernels) are held to."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import radiometry_oracle as RO
from diffusionremotesensing_amd import radiometry as R

RANGES = [(0, 65535), (0, 10000), (123, 4567)]
ALL = np.arange(65536, dtype=np.uint16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("lo,hi", RANGES)
def test_round_trip_of_all_65536_values(lo, hi):
    """quantise(normalise(v)) == v for every v in [lo, hi] (the error budget: span 2^-23 << 0.5), values outside clamp to the
    ends; the package's numpy forms have the oracle's bits."""
    table = [(lo, hi)]
    x = RO.normalise(ALL[None], table)
    assert x.dtype == np.float32 and x.min() == 0.0 and x.max() == 1.0
    back = RO.quantize(x, table)
    assert back.dtype == np.uint16
    want = np.clip(ALL.astype(np.int64), lo, hi).astype(np.uint16)
    assert np.array_equal(back[0], want)
    assert np.array_equal(back[0, lo:hi + 1], ALL[lo:hi + 1])
    assert np.array_equal(_bits(R.normalise_host(ALL[None], table)), _bits(x))
    assert np.array_equal(R.quantize_host(x, table), back)
    # strictly increasing inside the range: no two digital numbers share a float
    assert (np.diff(x[0, lo:hi + 1]) > 0).all()


def test_half_way_cases_round_to_even():
    x = np.array([[0.125, 0.375, 0.625, 0.875]], dtype=np.float32)  # * 4 = 0.5, 1.5, 2.5, 3.5
    for q in (RO.quantize, R.quantize_host):
        assert q(x, [(0, 4)]).tolist() == [[0, 2, 2, 4]]
        assert q(x, [(7, 11)]).tolist() == [[8, 8, 10, 10]]  # 7.5, 8.5, 9.5, 10.5
        assert q(np.array([[0.25, 0.75]], dtype=np.float32), [(100, 102)]).tolist() == [[100, 102]]


def test_nan_inf_and_negative_zero():
    x = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 1.5, -3.0]], dtype=np.float32)
    for q in (RO.quantize, R.quantize_host):
        assert q(x, [(123, 4567)]).tolist() == [[0, 4567, 123, 123, 123, 4567, 4567, 123]]
        assert q(x, [(123, 4567)], fill=65535).tolist()[0][0] == 65535
    with pytest.raises(ValueError, match="fill"):
        R.quantize_host(x, [(0, 1)], fill=65536)
    # per-band tables along the band axis
    v = np.array([[[5, 10]], [[5, 10]]], dtype=np.uint16)  # (C = 2, 1, 2)
    got = R.normalise_host(v, [(0, 10), (5, 15)])
    assert got.tolist() == [[[0.5, 1.0]], [[0.0, 0.5]]]
    assert np.array_equal(_bits(got), _bits(RO.normalise(v, [(0, 10), (5, 15)])))
    assert np.array_equal(R.normalise_host(np.moveaxis(v, 0, -1), [(0, 10), (5, 15)], band_axis=-1), np.moveaxis(got, 0, -1))


def test_tables_are_checked():
    assert R.check_table([(0, 65535)]).dtype == np.float32 and R.range_table([(1, 2)], 3).tolist() == [[1, 2]] * 3
    for bad in ([(5, 5)], [(6, 5)], [(-1, 5)], [(0, 65536)], [(0, float("nan"))], [0, 1], [(0, 1)] * 17):
        with pytest.raises(ValueError, match="data range"):
            R.check_table(bad)
    with pytest.raises(ValueError, match="names 2 bands, the images have 3"):
        R.range_table([(0, 1), (0, 2)], 3)


def test_percentiles_are_exact_order_statistics():
    rng = np.random.default_rng(5)
    n = 1000
    band0 = rng.integers(0, 65536, n)
    band1 = np.minimum(rng.gamma(2.0, 300.0, n), 65535).astype(np.int64)  # a few hundred values carry most pixels
    band2 = np.full(n, 500)
    band2[137] = 900  # all one value except one pixel
    cache = np.stack([band0, band1, band2]).astype(np.uint16).reshape(1, 3, 20, 50)
    counts = RO.histogram(cache)
    assert counts.sum(axis=1).tolist() == [n] * 3
    for plo, phi in ((0.0, 100.0), (2.0, 98.0), (0.5, 99.5), (10.0, 10.1 + 1e-9)):
        for c in (0, 1):
            want = [np.quantile(cache[0, c].reshape(-1), p / 100, method="lower") for p in (plo, phi)]
            if want[0] == want[1]:
                continue
            got = R.range_from_counts(counts[c:c + 1], plo, phi)
            assert got.dtype == np.float32 and got.tolist() == [want], (plo, phi, c)
            assert got.tolist() == RO.range_from_counts(counts[c:c + 1], plo, phi).tolist()
    assert R.range_from_counts(counts[2:], 0.0, 100.0).tolist() == [[500, 900]]
    with pytest.raises(ValueError, match="band 2: the 0.5th and 99.5th percentiles coincide at 500"):
        R.range_from_counts(counts)
    with pytest.raises(ValueError, match="no counted pixel"):
        R.range_from_counts(np.zeros((1, 65536), dtype=np.int64))
    # a torch tensor of counts, as the launch returns it
    assert R.range_from_counts(torch.from_numpy(counts[:2]), 2.0, 98.0).tolist() == RO.range_from_counts(counts[:2], 2.0, 98.0).tolist()
    # rank floor(p / 100 (n - 1)): two pixels, the upper one only at p = 100
    two = np.zeros((1, 65536), dtype=np.int64)
    two[0, 3] = two[0, 9] = 1
    assert R.range_from_counts(two, 0.0, 100.0).tolist() == [[3, 9]]
    with pytest.raises(ValueError, match="coincide at 3"):
        R.range_from_counts(two, 0.0, 99.9)
    assert R.reduce_counts(torch.from_numpy(two)) is not None  # (no process group: the counts themselves)


def test_data_range_parsing():
    assert R.parse_data_range("0,10000") == ("fixed", [(0.0, 10000.0)])
    assert R.parse_data_range("0,10000;123,4567") == ("fixed", [(0.0, 10000.0), (123.0, 4567.0)])
    assert R.parse_data_range("auto") == ("auto", 0.5, 99.5) and R.parse_data_range("auto:1,99") == ("auto", 1.0, 99.0)
    assert R.parse_data_range(R.DEFAULT_RANGE) == ("fixed", [(0.0, 65535.0)])
    for bad in ("", "1", "1,2,3", "5,5", "0,70000", "auto:", "auto:5", "auto:60,40", "auto:0,101", "autox", "a,b", "0,1;"):
        with pytest.raises(ValueError, match="data.range"):
            R.parse_data_range(bad)
    assert R.format_table([(0, 10000), (123, 4567.5)]) == "0,10000;123,4567.5"


def _write_u16_folder(root, names, size, bands=3, seed=0):
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    out = {}
    for name in names:
        out[name] = rng.integers(0, 65536, (size, size, bands)).astype(np.uint16)
        np.save(os.path.join(root, name + ".npy"), out[name])
    return out


def test_loader(tmp_path, capsys):
    from PIL import Image
    root = str(tmp_path / "a")
    files = _write_u16_folder(root, ["d", "b", "a", "c", "e"], 6)
    got = R.load_folder_u16(root, 6)
    assert got.dtype == torch.uint16 and tuple(got.shape) == (5, 3, 6, 6)
    for i, name in enumerate("abcde"):  # sorted order, HWC -> CHW
        assert np.array_equal(got[i].numpy(), np.moveaxis(files[name], -1, 0))
    # sharding: every world-th file, equal shards, the remainder left out and counted on rank 0
    r0, r1 = R.load_folder_u16(root, 6, 0, 2), R.load_folder_u16(root, 6, 1, 2)
    assert "1 of 5 images left out" in capsys.readouterr().out
    assert np.array_equal(r0.numpy(), got[[0, 2]].numpy()) and np.array_equal(r1.numpy(), got[[1, 3]].numpy())
    assert np.array_equal(R.load_folder_u16(root, 6, 1, 2, limit=3).numpy(), got[:3].numpy())
    with pytest.raises(ValueError, match="cannot be sharded over 6 ranks"):
        R.load_folder_u16(root, 6, 0, 6)
    # (H, W) arrays and I;16 PNGs are single bands
    root = str(tmp_path / "b")
    os.makedirs(root)
    rng = np.random.default_rng(1)
    plane, png = rng.integers(0, 65536, (6, 6)).astype(np.uint16), rng.integers(0, 65536, (6, 6)).astype(np.uint16)
    png[0, :3] = 0, 65535, 256
    np.save(os.path.join(root, "0.npy"), plane)
    Image.fromarray(png).save(os.path.join(root, "1.png"))
    with Image.open(os.path.join(root, "1.png")) as f:
        assert f.mode == "I;16"
    got = R.load_folder_u16(root, 6)
    assert tuple(got.shape) == (2, 1, 6, 6) and np.array_equal(got[0, 0].numpy(), plane) and np.array_equal(got[1, 0].numpy(), png)


def test_loader_refusals(tmp_path):
    from PIL import Image

    def folder(name, **files):
        root = str(tmp_path / name)
        os.makedirs(root)
        for fname, a in files.items():
            if fname.endswith("png"):
                Image.fromarray(a).save(os.path.join(root, fname.replace("_", ".")))
            else:
                np.save(os.path.join(root, fname + ".npy"), a)
        return root
    ok = np.zeros((6, 6, 3), dtype=np.uint16)
    with pytest.raises(ValueError, match=r"b\.npy: expected a uint16 array of digital numbers, got float32"):
        R.load_folder_u16(folder("float", a=ok, b=np.zeros((6, 6, 3), dtype=np.float32)), 6)
    with pytest.raises(ValueError, match=r"b\.npy: 2 bands, the files before it have 3"):
        R.load_folder_u16(folder("mixed", a=ok, b=np.zeros((6, 6, 2), dtype=np.uint16)), 6)
    with pytest.raises(ValueError, match=r"b\.npy: 6 x 8 pixels, the cache is 6 x 6: there is no 16-bit resize"):
        R.load_folder_u16(folder("size", a=ok, b=np.zeros((6, 8, 3), dtype=np.uint16)), 6)
    with pytest.raises(ValueError, match=r"a\.npy: 6 x 6 pixels, the cache is 8 x 8"):
        R.load_folder_u16(folder("size2", a=ok), 8)
    with pytest.raises(ValueError, match=r"a\.npy: expected one \(H, W, C\) or \(H, W\) array"):
        R.load_folder_u16(folder("bands", a=np.zeros((6, 6, 17), dtype=np.uint16)), 6)
    with pytest.raises(ValueError, match=r"a\.png: image mode 'L' is not a single-band 16-bit image"):
        R.load_folder_u16(folder("eight", a_png=np.zeros((6, 6), dtype=np.uint8)), 6)
    root = folder("junk", a=ok)
    with open(os.path.join(root, "b.txt"), "w") as f:
        f.write("no image")
    with pytest.raises(ValueError, match=r"b\.txt: not an image Pillow can read"):
        R.load_folder_u16(root, 6)


def test_synthetic_u16_is_the_rounded_patches():
    hr = torch.tensor([[[[0.0, 0.12344, 0.99996, 1.0]]]])
    assert R.synthetic_u16(hr).dtype == torch.uint16 and R.synthetic_u16(hr).numpy().tolist() == [[[[0, 1234, 10000, 10000]]]]


# ---- command lines -----------------------------------------------------------------------------------------------------------
def test_trainer_flags_and_refusals(capsys):
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    args = sr.parse_train_args([])
    assert args.bit_depth == 8 and args.data_range is None
    args = sr.parse_train_args(["--bit_depth", "16", "--data_range", "auto", "--nodata", "65535", "--dataset_path", "synthetic_u16:8"])
    assert args.bit_depth == 16 and args.data_range == "auto" and args.nodata == 65535
    assert sr.parse_train_args(["--bit_depth", "16", "--data_range", "0,10000;5,6"]).data_range == "0,10000;5,6"
    capsys.readouterr()
    for argv, words in (
            (["--data_range", "0,10000"], "--data_range belongs to --bit_depth 16"),
            (["--bit_depth", "12"], "invalid choice"),
            (["--bit_depth", "16", "--data_range", "5,5"], "0 <= LO < HI <= 65535"),
            (["--bit_depth", "16", "--data_range", "auto:60,40"], "0 <= PLO < PHI <= 100"),
            (["--bit_depth", "16", "--Degradation_type", "DownBlurNoise"], "its noise levels are defined on bytes"),
            (["--bit_depth", "16", "--Degradation_type", "BSRGAN"], "BSRGAN"),
            (["--bit_depth", "16", "--dataset_path", "synthetic_u8:4"], "not 'synthetic_u8:4'"),
            (["--dataset_path", "synthetic_u16:4"], "synthetic_u16 needs --bit_depth 16"),
            (["--nodata", "256"], "argument --nodata: '256' must lie in 0 .. 255"),
            (["--bit_depth", "16", "--nodata", "65536"], "must lie in 0 .. 65535"),
            (["--bit_depth", "16", "--nodata", "0.5"], "must be an integer")):
        with pytest.raises(SystemExit):
            sr.parse_train_args(argv)
        assert words in capsys.readouterr().err, argv
    # registered without a --help entry: the trainer's help text is recorded
    with pytest.raises(SystemExit):
        sr.parse_train_args(["--help"])
    out = capsys.readouterr().out
    assert "--bit_depth" not in out and "--data_range" not in out
    # `launch` refuses the same before it touches a device
    args = sr.parse_train_args(["--bit_depth", "16"])
    args.Degradation_type = "DownBlurNoise"
    with pytest.raises(ValueError, match="defined on bytes"):
        sr.launch(args)


def test_evaluate_and_tiler_flags():
    from diffusionremotesensing_amd import Aggregation_Sampling as A
    from diffusionremotesensing_amd import evaluate
    p = evaluate.cli_arg_parser("superres")
    assert "--bit_depth" in p.format_help() and "--data_range" in p.format_help()
    args = p.parse_args(["--bit_depth", "16", "--data_range", "0,10000", "--nodata", "4000"])
    assert (args.bit_depth, args.data_range, args.nodata) == (16, "0,10000", 4000) and evaluate._evaluate_nodata(args, "superres") is True
    assert p.parse_args([]).bit_depth == 8
    assert "--bit_depth" not in evaluate.cli_arg_parser("sar_to_ndvi").format_help()
    with pytest.raises(ValueError, match="belongs to --bit_depth 16"):
        R.check_args(p.parse_args(["--data_range", "auto"]))
    t = A.build_arg_parser().parse_args(["--out_u16", "--data_range", "0,10000"])
    assert t.out_u16 is True and t.data_range == "0,10000" and A.build_arg_parser().parse_args([]).out_u16 is False


# ---- snapshots and the train state -------------------------------------------------------------------------------------------
def _stub(tmp_path, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", nn.Linear(3, 2), str(tmp_path / "run" / "snapshot.pt"), noise_steps=10, device="cpu", image_size=8,
                     magnification_factor=2, Degradation_type="DownBlur", **kw)


def _train(d, **kw):
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=[], val_loader=None, patience=5, loss="MSE", verbose=False, **kw)
    return d


def test_data_range_in_snapshot_and_resume_mismatch(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "run")
    monkeypatch.setattr(torch.cuda, "get_rng_state", lambda device=None: torch.zeros(1, dtype=torch.uint8))
    snap, state = str(tmp_path / "run" / "snapshot.pt"), str(tmp_path / "run" / "train_state.pt")
    # an 8-bit run writes the files it always wrote
    d = _train(_stub(tmp_path), save_train_state=True)
    assert d.data_range is None and d.snapshot_data_range is None
    assert "DATA_RANGE" not in torch.load(snap) and "DATA_RANGE" not in torch.load(state)
    # ... and a 16-bit run does not go on from them
    d = _stub(tmp_path)
    d.data_range = R.range_table([(0, 10000)], 3)
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --data_range none \(an 8-bit run\), this run has 0,10000;0,10000;0,10000"):
        _train(d)
    os.remove(snap), os.remove(state)
    table = R.check_table([(0, 10000), (123, 4567), (5, 60000)])
    d = _stub(tmp_path)
    d.data_range = table
    _train(d, save_train_state=True)
    for path in (snap, state):
        saved = torch.load(path)["DATA_RANGE"]
        assert saved.dtype == torch.float32 and saved.tolist() == table.tolist()
    d = _stub(tmp_path)  # what evaluate and the tiler read
    assert d.snapshot_data_range.tolist() == table.tolist() and d.data_range is None
    d.data_range = torch.from_numpy(table)  # the same table, as a tensor: goes on
    _train(d, save_train_state=True)
    other = table.copy()
    other[1, 1] = 4568
    d = _stub(tmp_path)
    d.data_range = other
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --data_range 0,10000;123,4567;5,60000, this run has 0,10000;123,4568"):
        _train(d)
    d = _stub(tmp_path)  # an 8-bit run on a 16-bit snapshot
    with pytest.raises(ValueError, match="this run has none"):
        _train(d)
    # train_state.pt alone disagrees
    ts = torch.load(state)
    ts["DATA_RANGE"] = torch.from_numpy(other)
    torch.save(ts, state)
    d = _stub(tmp_path)
    d.data_range = table
    with pytest.raises(ValueError, match=r"train_state\.pt was written with --data_range 0,10000;123,4568"):
        _train(d, save_train_state=True)


def test_launcher_sets_data_range():
    from diffusionremotesensing_amd import launcher
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    made = []

    class D:
        data_range = None

        def __init__(self, **kw):
            made.append(self)

        def train(self, **kw):
            self.seen_at_train = self.data_range
    args = sr.parse_train_args(["--bit_depth", "16"])
    args.snapshot_folder_path = "."
    table = R.range_table([(0, 10000)], 3)
    launcher.train_model(args, D, nn.Linear(2, 2), "cpu", [], None)
    launcher.train_model(args, D, nn.Linear(2, 2), "cpu", [], None, data_range=table)
    assert made[0].seen_at_train is None and made[1].seen_at_train is table


def test_feed_refusals_need_no_device():
    u16 = torch.zeros((2, 3, 8, 8), dtype=torch.uint16)
    feed = R.DeviceU16SuperresFeed(u16, 2, 0.5, 2, False, None)
    assert feed.data_range.tolist() == [[0, 65535]] * 3 and len(feed) == 1 and feed.blur_radius == 0.5 and feed.last_items is None
    assert feed.operator.hr_shape == (8, 8) and feed.operator.lr_shape == (4, 4)
    assert len(R.DeviceU16SuperresFeed(u16, 2, 0.5, 2, False, None, crop_size=4, augment="d4", num_crops=3)) == 3
    r = R.DeviceU16SuperresFeed(u16, 2, "random", 2, False, None).blur_radius
    assert 0.5 <= r <= 1.5
    with pytest.raises(RuntimeError, match="torch.uint16"):
        R.DeviceU16SuperresFeed(u16.to(torch.uint8), 2, 0.5, 2, False, None)
    with pytest.raises(ValueError, match="square windows"):
        R.DeviceU16SuperresFeed(torch.zeros((2, 3, 8, 10), dtype=torch.uint16), 2, 0.5, 2, False, None)
    with pytest.raises(ValueError, match="names 2 bands, the images have 3"):
        R.DeviceU16SuperresFeed(u16, 2, 0.5, 2, False, [(0, 1), (0, 2)])
    with pytest.raises(ValueError, match="nodata=65536"):
        R.DeviceU16SuperresFeed(u16, 2, 0.5, 2, False, None, nodata=65536)
    with pytest.raises(RuntimeError, match="ROCm device"):
        R.hist_u16(u16)
    assert math.isclose(feed.operator.A_y.sum(axis=1).max(), 1.0, rel_tol=1e-12)
