"""The two gather kernels of csrc/feed.hip and the device feeds built on them (diffusionremotesensing_amd/feeds.py), bit for
bit: the formulas are single fp32 operations, so the bar is equality.  Then one epoch of the SAR -> NDVI and the generation
trainers on dataset folders, and the evaluate command on the SAR snapshot.

Expected values come from the host, computed with the reference's own expressions - `(img + 1) / 2` (utils.py:88-89) and
ToTensor's `.float().div(255)`, both CPU operations there.  Both kernels are also held against torch on the device: the pair
kernel against the same expression, the byte kernel against a division by a 255 TENSOR.  `x.div(255)` with the Python scalar is
only printed there: torch's device kernel for it multiplies by the rounded reciprocal (its source says this may lose a bit; 126
of the 256 byte values differ from the true quotient), which is not what ToTensor computes on the host."""
import json
import math
import os

import pytest
import torch

from feeds_fixtures import GOLDEN_FEEDS, golden_items, write_class_tree, write_sar_folder

pytestmark = pytest.mark.gpu

L = 3
SHAPES = [(1, 5, 7),     # rows of 35 elements: every row after the first starts unaligned, odd tail
          (2, 8, 8),     # rows of 128 elements: every row aligned
          (3, 32, 32)]   # rows of 3072 elements: several blocks per row
IDX = {1: [2], 5: [2, 1, 2, 1, 0]}  # repeats; with 35-element rows: rows aligned alike with heads of 0, 1 and 2 floats, and not


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _f32_cache(shape, seed):
    """(L, C, H, W) fp32 in [-1.5, 1.5] with the exact values -1, 0 and 1."""
    x = torch.rand((L,) + shape, generator=torch.Generator().manual_seed(seed)) * 3 - 1.5
    x.view(L, -1)[:, :3] = torch.tensor([-1.0, 0.0, 1.0])
    return x


def _u8_cache(shape, seed):
    """(L, C, H, W) uint8: a seeded shuffle of 0, 1, 2, ... (mod 256), so every byte value occurs once there are 256 elements."""
    n = L * shape[0] * shape[1] * shape[2]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return (torch.arange(n)[perm] % 256).to(torch.uint8).view((L,) + shape)


# ---------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("pair", [0, 1, 2])
def test_gather_pairs_bit_exact(dev, pair, n):
    from diffusionremotesensing_amd.feeds import gather_pairs
    sar, ndvi = _f32_cache(SHAPES[pair], 10 + pair), _f32_cache(SHAPES[(pair + 1) % 3], 20 + pair)
    idx = torch.tensor(IDX[n], dtype=torch.int64)
    sar_d, ndvi_d, idx_d = sar.to(dev), ndvi.to(dev), idx.to(dev)
    got_sar, got_ndvi = gather_pairs(sar_d, ndvi_d, idx_d)
    assert got_sar.shape == (n,) + SHAPES[pair] and got_ndvi.shape == (n,) + SHAPES[(pair + 1) % 3]
    assert torch.equal(got_sar.cpu(), (sar[idx] + 1) / 2) and torch.equal(got_ndvi.cpu(), (ndvi[idx] + 1) / 2)
    assert torch.equal(got_sar, (sar_d[idx_d] + 1) / 2) and torch.equal(got_ndvi, (ndvi_d[idx_d] + 1) / 2)
    assert float(got_sar.min()) < 0 and float(got_sar.max()) > 1  # nothing is clipped: values outside [-1, 1] pass through


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_u8_bit_exact(dev, shape, n):
    from diffusionremotesensing_amd.feeds import gather_u8
    u8 = _u8_cache(shape, 30 + shape[0])
    if u8.numel() >= 256:
        assert u8.unique().numel() == 256
    labels = torch.tensor([7, -3, 2 ** 40 + 5], dtype=torch.int64)
    idx = torch.tensor(IDX[n], dtype=torch.int64)
    u8_d, idx_d = u8.to(dev), idx.to(dev)
    img, lab = gather_u8(u8_d, labels.to(dev), idx_d)
    assert img.shape == (n,) + shape and img.dtype == torch.float32 and lab.dtype == torch.int64
    assert torch.equal(img.cpu(), u8[idx].float().div(255))
    assert torch.equal(lab.cpu(), labels[idx])
    # on the device the same quotient is a division by a TENSOR (correctly rounded, like the host's); by the Python scalar 255
    # torch multiplies by the reciprocal there, which is printed for the record
    assert torch.equal(img, u8_d[idx_d].float() / torch.tensor(255.0, device=dev))
    print(f"u8 {shape} n={n}: {int((img != u8_d[idx_d].float().div(255)).sum())} of {img.numel()} elements differ from torch's "
          "device-side .div(255)")


def test_gather_u8_all_byte_values_in_one_row(dev):
    """Every byte value, in order, at an aligned start: the quotients of the whole table."""
    from diffusionremotesensing_amd.feeds import gather_u8
    u8 = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16)
    img, _ = gather_u8(u8.to(dev), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))
    assert torch.equal(img.cpu(), u8.float().div(255))


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_out_of_range_index_gives_a_zero_row(dev, shape):
    from diffusionremotesensing_amd.feeds import gather_pairs, gather_u8
    idx = torch.tensor([1, L, 0, -1, 2], dtype=torch.int64)
    ok = torch.tensor([True, False, True, False, True])
    safe = idx.clamp(0, L - 1)
    sar, ndvi, u8 = _f32_cache(shape, 40), _f32_cache(SHAPES[2], 41), _u8_cache(shape, 42)
    labels = torch.tensor([11, 12, 13], dtype=torch.int64)
    got_sar, got_ndvi = gather_pairs(sar.to(dev), ndvi.to(dev), idx.to(dev))
    img, lab = gather_u8(u8.to(dev), labels.to(dev), idx.to(dev))
    mask = ok.view(-1, 1, 1, 1)
    assert torch.equal(got_sar.cpu(), torch.where(mask, (sar[safe] + 1) / 2, torch.zeros(())))
    assert torch.equal(got_ndvi.cpu(), torch.where(mask, (ndvi[safe] + 1) / 2, torch.zeros(())))
    assert torch.equal(img.cpu(), torch.where(mask, u8[safe].float().div(255), torch.zeros(())))
    assert lab.cpu().tolist() == [12, -1, 11, -1, 13]


def test_rows_past_two_gib(dev):
    """Cache offsets beyond 2^31 bytes (u8) and 2^31 elements (fp32): the last row of a cache of 2049 rows of 2^20 elements.
    The caches are allocated, not filled: only the rows that are read are written."""
    from diffusionremotesensing_amd.feeds import gather_pairs, gather_u8
    big, shape = 2049, (1, 1024, 1024)
    gen = torch.Generator().manual_seed(50)
    idx = torch.tensor([big - 1, 0], dtype=torch.int64)
    rows_u8 = torch.randint(0, 256, (2,) + shape, generator=gen, dtype=torch.uint8)
    u8 = torch.empty((big,) + shape, dtype=torch.uint8, device=dev)
    u8[big - 1], u8[0] = rows_u8[0].to(dev), rows_u8[1].to(dev)
    labels = torch.arange(big, dtype=torch.int64, device=dev)
    img, lab = gather_u8(u8, labels, idx.to(dev))
    assert torch.equal(img.cpu(), rows_u8.float().div(255)) and lab.cpu().tolist() == [big - 1, 0]
    del u8, img
    rows = torch.rand((2,) + shape, generator=gen) * 2 - 1
    sar = torch.empty((big,) + shape, dtype=torch.float32, device=dev)
    sar[big - 1], sar[0] = rows[0].to(dev), rows[1].to(dev)
    ndvi = torch.arange(big, dtype=torch.float32, device=dev).view(big, 1, 1, 1)
    got_sar, got_ndvi = gather_pairs(sar, ndvi, idx.to(dev))
    assert torch.equal(got_sar.cpu(), (rows + 1) / 2)
    assert got_ndvi.flatten().cpu().tolist() == [big / 2, 0.5]
    del sar, got_sar
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------
# feeds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,data_format", [("pt", "torch"), ("npy", "numpy")])
def test_sar_feed_gives_the_reference_items(dev, fmt, data_format):
    from diffusionremotesensing_amd.feeds import DeviceSarNdviFeed, load_sar_ndvi_folder
    items, _ = golden_items()
    sar, ndvi = load_sar_ndvi_folder(os.path.join(GOLDEN_FEEDS, fmt, "train"), data_format)
    feed = DeviceSarNdviFeed(sar.to(dev), ndvi.to(dev), batch_size=2, shuffle=False)
    batches = list(feed)
    assert len(feed) == len(batches) == 2 and [b[0].shape[0] for b in batches] == [2, 1]
    got_sar, got_ndvi = torch.cat([b[0] for b in batches]).cpu(), torch.cat([b[1] for b in batches]).cpu()
    for i, (want_sar, want_ndvi) in enumerate(items):
        assert torch.equal(got_sar[i], want_sar) and torch.equal(got_ndvi[i], want_ndvi), i
        x, y = feed.item(i)
        assert torch.equal(x.cpu(), want_sar) and torch.equal(y.cpu(), want_ndvi)
    with pytest.raises(IndexError):
        feed.item(3)


def test_sar_feed_shuffles_like_a_seeded_loader(dev):
    from diffusionremotesensing_amd.evaluate import unshuffled
    from diffusionremotesensing_amd.feeds import DeviceSarNdviFeed
    n = 7
    # item k holds k in its SAR image and -k in its NDVI image: a batch tells which items it is made of
    ids = torch.arange(n, dtype=torch.float32).view(n, 1, 1, 1)
    sar, ndvi = (ids * 2 - 1).expand(n, 2, 4, 4).contiguous().to(dev), (-ids * 2 - 1).expand(n, 1, 4, 4).contiguous().to(dev)

    def epoch(feed):
        out = []
        for x, y in feed:
            assert x.shape[1:] == (2, 4, 4) and y.shape[1:] == (1, 4, 4) and x.is_cuda
            assert torch.equal(x[:, 0, 0, 0], -y[:, 0, 0, 0])  # the pair stays together
            out.append(x[:, 0, 0, 0].cpu().round().long())
        return out

    a = DeviceSarNdviFeed(sar, ndvi, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(3))
    b = DeviceSarNdviFeed(sar, ndvi, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(3))
    first, second, other = epoch(a), epoch(a), epoch(b)
    assert [len(v) for v in first] == [3, 3, 1] and len(a) == 3
    assert sorted(torch.cat(first).tolist()) == list(range(n)) == sorted(torch.cat(second).tolist())
    assert torch.equal(torch.cat(first), torch.randperm(n, generator=torch.Generator().manual_seed(3)))
    assert torch.equal(torch.cat(first), torch.cat(other))
    assert not torch.equal(torch.cat(first), torch.cat(second))  # the generator moves on: a new order every epoch
    assert unshuffled(a) is a and torch.cat(epoch(a)).tolist() == list(range(n))


def test_class_feed(dev, tmp_path):
    from diffusionremotesensing_amd.feeds import DeviceClassFeed, load_class_folder_u8
    root = str(tmp_path / "tree")
    write_class_tree(root, 8)
    u8, labels, classes = load_class_folder_u8(root, 8)
    want = u8.float().div(255)
    feed = DeviceClassFeed(u8.to(dev), labels.to(dev), classes, batch_size=2, shuffle=False)
    batches = list(feed)
    assert [b[0].shape[0] for b in batches] == [2, 2, 1] and all(b[0].is_cuda and b[1].is_cuda for b in batches)
    assert torch.equal(torch.cat([b[0] for b in batches]).cpu(), want)
    assert torch.equal(torch.cat([b[1] for b in batches]).cpu(), labels)
    # what the reference's launch reads from the loader
    assert feed.dataset.classes == classes == feed.classes and len(feed.dataset) == 5
    img, label = feed.dataset[3]
    assert img.shape[0] == 3 and torch.equal(img.cpu(), want[3]) and label == 1 and isinstance(label, int)
    shuffled = DeviceClassFeed(u8.to(dev), labels.to(dev), classes, batch_size=5, shuffle=True,
                               generator=torch.Generator().manual_seed(1))
    order = torch.randperm(5, generator=torch.Generator().manual_seed(1))
    (img5, lab5), = list(shuffled)
    assert torch.equal(img5.cpu(), want[order]) and torch.equal(lab5.cpu(), labels[order])


# ---------------------------------------------------------------------------------------------
# end to end, at the smallest shape the network takes
# ---------------------------------------------------------------------------------------------
_RUN = ["--image_size", "16", "--noise_steps", "10", "--epochs", "1", "--batch_size", "2", "--check_preds_epoch", "1",
        "--loss", "MSE"]


def test_sar_trainer_and_evaluate_on_a_folder(dev, tmp_path, monkeypatch, capsys):
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as S
    data = str(tmp_path / "data")
    write_sar_folder(os.path.join(data, "train"), ["d", "b", "a", "c"], 16, seed=1)
    write_sar_folder(os.path.join(data, "test"), ["y", "x"], 16, seed=2)
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    S.main(_RUN + ["--model_name", "sar_folder", "--dataset_path", data])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Training snapshot saved" in out
    assert os.path.exists(tmp_path / "models_run" / "sar_folder" / "weights" / "snapshot.pt")
    res = torch.load(tmp_path / "models_run" / "sar_folder" / "results" / "SAR_TO_NDVI_results.pt")
    assert tuple(res.shape) == (4, 1, 16, 16) and bool(torch.isfinite(res).all())  # train items 0..3: all there are
    scores = evaluate.main(["--task", "sar_to_ndvi", "--model_name", "sar_folder", "--image_size", "16", "--noise_steps", "10",
                            "--batch_size", "2", "--dataset_path", data, "--n_images", "2", "--sampling_steps", "4",
                            "--out", str(tmp_path / "sar.json")])
    out = capsys.readouterr().out
    assert "PSNR" in out and "SSIM" in out and "wrote" in out
    saved = json.load(open(tmp_path / "sar.json"))
    assert saved["n"] == scores["n"] == 2 and set(saved) == {"model", "per_image", "n", "args"}
    assert set(saved["model"]) == {"psnr", "ssim"}  # one NDVI band: no spectral angle
    assert all(math.isfinite(v) for v in saved["model"].values()), saved["model"]
    assert all(len(v) == 2 for v in saved["per_image"]["model"].values())
    with pytest.raises(ValueError, match="--image_size is 8"):
        S.main(["--image_size", "8"] + _RUN[2:] + ["--model_name", "sar_folder8", "--dataset_path", data])


def test_generation_trainer_on_a_class_folder(dev, tmp_path, monkeypatch, capsys):
    import numpy as np
    from PIL import Image
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as G
    rng = np.random.default_rng(3)
    for cls in ("water", "forest"):
        os.makedirs(tmp_path / "tree" / cls)
        for k in range(2):
            Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(tmp_path / "tree" / cls / f"{k}.png")
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    np.random.seed(0)
    G.main(_RUN + ["--model_name", "gen_folder", "--dataset_path", str(tmp_path / "tree")])
    out = capsys.readouterr().out
    assert "Epoch 0 | Training snapshot saved" in out and "Running Val loss" not in out  # no validation set, as in the reference
    snap = torch.load(tmp_path / "models_run" / "gen_folder" / "weights" / "snapshot.pt", map_location="cpu")
    assert snap["EPOCHS_RUN"] == 0 and snap["MODEL_STATE"]["label_emb.weight"].shape[0] == 2
    res = torch.load(tmp_path / "models_run" / "gen_folder" / "results" / "generation_results.pt")
    assert tuple(res.shape) == (10, 3, 16, 16) and bool(torch.isfinite(res).all())
