"""PSNR / SSIM / SAM / ERGAS on the GPU (csrc/metrics.hip through diffusionremotesensing_amd.metrics) against the float64
oracle of tests/metrics_oracle.py, `Diffusion.evaluate` of both conditional models, the evaluate command and the trainer's
--eval_metrics hook."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import metrics_oracle as MO
from conftest import replay_noise_source

pytestmark = pytest.mark.gpu

# One tenth of the last digit the evaluate command prints: requirements, not measurements.
TOL_PSNR_DB, TOL_SSIM, TOL_SAM_DEG, TOL_SAM_REL, TOL_ERGAS_REL = 1e-3, 1e-5, 1e-4, 1e-4, 1e-5
MAG = 2

SHAPES = [(1, 1, 11, 11),   # a single window position
          (2, 3, 12, 27),   # odd width, H * W % 4 != 0 (the scalar instance), tiles overhanging
          (3, 13, 33, 47),  # 13 bands
          (2, 16, 64, 72),  # 16 bands, several SSIM tiles in both directions
          (1, 3, 64, 64)]
CONTENTS = ["noise", "smooth_1e-2", "smooth_1e-3", "bright_flat", "identical"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _pair(shape, content, seed=0):
    """(sr, hr) fp32 CPU tensors of one test content."""
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + 17 * CONTENTS.index(content))
    B, C, H, W = shape
    if content == "noise":  # uniform in [-0.2, 1.2]: the clamp matters, zero pixels occur with few bands
        return tuple(torch.rand(shape, generator=g) * 1.4 - 0.2 for _ in range(2))
    if content.startswith("smooth"):
        hr = F.interpolate(torch.rand((B, C, 8, 8), generator=g), size=(H, W), mode="bicubic", align_corners=False)
        return hr + float(content.split("_")[1]) * torch.randn(shape, generator=g), hr
    if content == "bright_flat":
        return tuple(0.95 + 0.002 * torch.randn(shape, generator=g) for _ in range(2))
    hr = torch.rand(shape, generator=g)
    return hr.clone(), hr


def _errors(got, want):
    """{metric: worst error over the batch in the unit of its tolerance's test} and the pass / fail of each."""
    errs, ok = {}, {}
    for k in want:
        g, w = got[k].cpu(), want[k]
        assert g.dtype == torch.float64 and g.shape == w.shape, k
        same = (g == w) | (torch.isnan(g) & torch.isnan(w))  # inf == inf, NaN where the oracle has NaN
        d = torch.where(same, torch.zeros_like(w), (g - w).abs())
        if k == "sam":
            bound = torch.maximum(torch.full_like(w, TOL_SAM_DEG), TOL_SAM_REL * w.abs())
        elif k == "ergas":
            bound = TOL_ERGAS_REL * w.abs()
        else:
            bound = torch.full_like(w, TOL_PSNR_DB if k == "psnr" else TOL_SSIM)
        bound = torch.where(same, torch.zeros_like(w), bound)
        errs[k] = (d / w.abs().clamp_min(1e-300)).max().item() if k == "ergas" else d.max().item()
        ok[k] = bool((d <= bound).all())
    return errs, ok


def _assert_matches_oracle(got, want, what):
    errs, ok = _errors(got, want)
    assert set(got) == set(want), (set(got), set(want))
    assert all(ok.values()), (what, errs)
    return errs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_vs_float64_oracle(dev, shape):
    """`image_quality` on five contents per shape against the float64 oracle: PSNR <= 1e-3 dB, SSIM <= 1e-5, SAM <=
    max(1e-4 degrees, 1e-4 relative), ERGAS <= 1e-5 relative; identical images give exactly inf, 1.0, 0.0 and 0.0.
    Measured on MI355X, worst over the five contents, (1,1,11,11) / (2,3,12,27) / (3,13,33,47) / (2,16,64,72) / (1,3,64,64):
    PSNR 2.1e-7 / 1.2e-7 / 4.3e-8 / 8.0e-8 / 1.7e-7 dB, SSIM 7.9e-7 / 1.0e-7 / 3.1e-8 / 4.8e-8 / 6.4e-8,
    SAM - / 1.2e-6 / 1.6e-6 / 1.2e-6 / 8.7e-7 degrees, ERGAS 6.0e-8 / 3.5e-8 / 1.4e-8 / 1.6e-8 / 3.1e-8 relative."""
    from diffusionremotesensing_amd import metrics
    worst = {}
    for content in CONTENTS:
        sr, hr = _pair(shape, content)
        got = metrics.image_quality(sr.to(dev), hr.to(dev), MAG)
        want = MO.image_quality(sr, hr, MAG)
        assert ("sam" in got) == (shape[1] >= 2)
        errs = _assert_matches_oracle(got, want, (shape, content))
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        if content == "identical":
            assert torch.isinf(got["psnr"]).all() and (got["psnr"] > 0).all()
            assert (got["ssim"] == 1.0).all() and (got["ergas"] == 0.0).all()
            assert shape[1] < 2 or (got["sam"] == 0.0).all()
    print(f"metrics {shape}: worst errors " + " ".join(f"{k} {e:.2e}" for k, e in worst.items()))


def test_zero_pixels_occur_and_are_left_out(dev):
    """The clamped noise of the 3-band case holds pixels whose vector is exactly zero; the kernel's count leaves them out."""
    from diffusionremotesensing_amd import hip_ops
    sr, hr = _pair((2, 3, 12, 27), "noise")
    zero = ((sr.clamp(0, 1) == 0).all(dim=1) | (hr.clamp(0, 1) == 0).all(dim=1)).sum(dim=(1, 2))
    assert int(zero.sum()) > 0
    sums = hip_ops.metrics_pointwise(sr.to(dev), hr.to(dev), clamp=True).cpu()
    assert sums.shape == (2, 8) and torch.equal(sums[:, 7], (12 * 27 - zero).double())


def test_without_clamp(dev):
    from diffusionremotesensing_amd import metrics
    for shape in SHAPES[1:4]:
        sr, hr = _pair(shape, "noise")
        got = metrics.image_quality(sr.to(dev), hr.to(dev), MAG, clamp=False)
        _assert_matches_oracle(got, MO.image_quality(sr, hr, MAG, clamp=False), shape)
        clamped = metrics.image_quality(sr.to(dev), hr.to(dev), MAG)
        assert not torch.equal(got["psnr"], clamped["psnr"]) and not torch.equal(got["ssim"], clamped["ssim"])


def test_image_without_a_valid_pixel_gives_nan_angle_only_there(dev):
    from diffusionremotesensing_amd import metrics
    sr, hr = _pair((3, 3, 12, 27), "smooth_1e-2")
    want = MO.image_quality(sr, hr, MAG)
    sr[1] = -0.5 * sr[1].abs()  # clamped to zero everywhere
    got = metrics.image_quality(sr.to(dev), hr.to(dev), MAG)
    assert math.isnan(got["sam"][1].item())
    assert all(math.isfinite(got[k][1].item()) for k in ("psnr", "ssim", "ergas"))
    _assert_matches_oracle(got, MO.image_quality(sr, hr, MAG), "zero image")
    for k in want:
        assert torch.equal(got[k].cpu()[[0, 2]], metrics.image_quality(sr[[0, 2]].to(dev), hr[[0, 2]].to(dev), MAG)[k].cpu())


@pytest.mark.parametrize("where", ["sr", "hr"])
def test_nan_stays_in_its_image(dev, where):
    from diffusionremotesensing_amd import metrics
    sr, hr = _pair((3, 3, 33, 47), "noise")
    clean = metrics.image_quality(sr.to(dev), hr.to(dev), MAG)
    (sr if where == "sr" else hr)[1, 2, 16, 20] = float("nan")
    got = metrics.image_quality(sr.to(dev), hr.to(dev), MAG)
    for k in ("psnr", "ssim", "sam", "ergas"):
        assert math.isnan(got[k][1].item()), k
        assert torch.equal(got[k][[0, 2]], clean[k][[0, 2]]), k


def test_repeatable_and_image_quality_equals_the_single_calls(dev):
    from diffusionremotesensing_amd import metrics
    for shape in SHAPES[1:4]:
        sr, hr = (t.to(dev) for t in _pair(shape, "smooth_1e-2"))
        a, b = metrics.image_quality(sr, hr, MAG), metrics.image_quality(sr, hr, MAG)
        single = {"psnr": metrics.psnr(sr, hr), "ssim": metrics.ssim(sr, hr), "sam": metrics.sam(sr, hr),
                  "ergas": metrics.ergas(sr, hr, MAG)}
        for k in single:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], single[k]), (shape, k)
    # a view whose planes are not 16-byte aligned takes the element-wise instance and agrees with the oracle
    sr, hr = _pair((2, 3, 16, 17), "smooth_1e-2")
    off_sr, off_hr = (t.to(dev).flatten()[1:1 + 2 * 3 * 16 * 16].view(2, 3, 16, 16) for t in (sr, hr))
    assert off_sr.data_ptr() % 16 != 0
    _assert_matches_oracle(metrics.image_quality(off_sr, off_hr, MAG), MO.image_quality(off_sr.cpu(), off_hr.cpu(), MAG), "offset")
    with pytest.raises(RuntimeError, match="same"):
        metrics.psnr(sr.to(dev), hr.to(dev)[:, :2])
    with pytest.raises(RuntimeError, match="status 2"):
        metrics.ssim(sr.to(dev)[:, :, :10], hr.to(dev)[:, :, :10])


# ---------------------------------------------------------------------------------------------
# Diffusion.evaluate
# ---------------------------------------------------------------------------------------------
T_STEPS, S_STEPS, SIZE = 8, 4, 64


def _superres(dev, sd):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, magnification_factor=MAG,
                  image_size=SIZE, Degradation_type="DownBlur")
    return m, d


def _stack(per_image):
    return {k: torch.tensor(v, dtype=torch.float64) for k, v in per_image.items()}


def test_evaluate_superres(dev, seeded_sd):
    """Two batches of two synthetic images, T = 8, DDIM S = 4: the per-image figures are the oracle's on the samples a direct
    `sample` call returns from the same noise, the bicubic block the oracle's on hip_ops.bicubic_upsample; n_images cuts."""
    from diffusionremotesensing_amd import hip_ops, synthetic
    m, d = _superres(dev, seeded_sd)
    hr = synthetic.tensor_uniform("metrics.hr", (4, 3, SIZE, SIZE))
    lr = synthetic.tensor_uniform("metrics.lr", (4, 3, SIZE // MAG, SIZE // MAG))
    loader = [(lr[:2], hr[:2]), (lr[2:], hr[2:])]
    res = d.evaluate(m, loader, sampling_steps=S_STEPS, noise_source=replay_noise_source(31))
    assert not m.training  # the model keeps its mode
    assert res["n"] == 4 and set(res) == {"model", "bicubic", "per_image", "n"}
    assert set(res["model"]) == set(res["bicubic"]) == {"psnr", "ssim", "sam", "ergas"}
    src = replay_noise_source(31)
    samples = []
    for lr_b, _ in loader:
        samples.append(d.sample(2, m, lr_b.to(dev), input_channels=3, noise_source=src, sampling_steps=S_STEPS).cpu())
        m.eval()
    samples = torch.cat(samples)
    assert not torch.equal(samples[0], samples[2])
    want = MO.image_quality(samples, hr, MAG)
    _assert_matches_oracle(_stack(res["per_image"]["model"]), want, "model")
    bic = hip_ops.bicubic_upsample(lr.to(dev), MAG).cpu()
    want_b = MO.image_quality(bic, hr, MAG)
    _assert_matches_oracle(_stack(res["per_image"]["bicubic"]), want_b, "bicubic")
    for name, w in (("model", want), ("bicubic", want_b)):
        for k, v in w.items():
            assert res[name][k] == pytest.approx(v.mean().item(), rel=1e-4, abs=1e-4), (name, k)
    three = d.evaluate(m, loader, n_images=3, sampling_steps=S_STEPS, noise_source=replay_noise_source(31), baseline=False)
    assert three["n"] == 3 and "bicubic" not in three and "bicubic" not in three["per_image"]
    for k, v in three["per_image"]["model"].items():
        assert len(v) == 3 and v[:2] == res["per_image"]["model"][k][:2] and math.isfinite(v[2]), k


def test_evaluate_sar_to_ndvi(dev, seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(seeded_sd_sar)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, image_size=SIZE)
    sar = synthetic.tensor_uniform("metrics.sar", (4, 2, SIZE, SIZE))
    ndvi = synthetic.tensor_uniform("metrics.ndvi", (4, 1, SIZE, SIZE))
    loader = [(sar[:2], ndvi[:2]), (sar[2:], ndvi[2:])]
    res = d.evaluate(m, loader, sampling_steps=S_STEPS, noise_source=replay_noise_source(32))
    assert res["n"] == 4 and set(res) == {"model", "per_image", "n"} and set(res["model"]) == {"psnr", "ssim"}
    src = replay_noise_source(32)
    samples = []
    for sar_b, _ in loader:
        samples.append(d.sample(2, m, sar_b.to(dev), NDVI_channels=1, noise_source=src, sampling_steps=S_STEPS).cpu())
        m.eval()
    _assert_matches_oracle(_stack(res["per_image"]["model"]), MO.image_quality(torch.cat(samples), ndvi), "sar")
    three = d.evaluate(m, loader, n_images=3, sampling_steps=S_STEPS, noise_source=replay_noise_source(32))
    assert three["n"] == 3 and len(three["per_image"]["model"]["psnr"]) == 3
    with pytest.raises(RuntimeError, match="batch of 2"):
        d.sample(3, m, sar[:2], NDVI_channels=1, sampling_steps=S_STEPS)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
_TRAIN = ["--epochs", "1", "--batch_size", "4", "--image_size", "32", "--noise_steps", "10", "--loss", "MSE",
          "--magnification_factor", "2", "--dataset_path", "synthetic:8", "--check_preds_epoch", "1", "--sampling_steps", "3"]


def test_evaluate_command_and_trainer_hook(dev, tmp_path, monkeypatch, capsys):
    """One trainer epoch with --eval_metrics 2 prints the metric line; `evaluate.main` on its snapshot prints the table and
    writes the JSON with the documented keys and finite values."""
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    T.main(_TRAIN + ["--model_name", "cli_metrics", "--eval_metrics", "2"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if "Val metrics" in ln]
    assert len(lines) == 1 and lines[0].startswith("Epoch 0: Val metrics on 2 images | model PSNR ")
    assert " | bicubic PSNR " in lines[0] and "SSIM" in lines[0] and "SAM" in lines[0] and "ERGAS" in lines[0]
    scores = evaluate.main(["--model_name", "cli_metrics", "--image_size", "32", "--noise_steps", "10", "--batch_size", "4",
                            "--magnification_factor", "2", "--dataset_path", "synthetic:4", "--sampling_steps", "3",
                            "--out", str(tmp_path / "r.json")])
    out = capsys.readouterr().out
    assert "PSNR" in out and "bicubic" in out and "wrote" in out
    saved = json.load(open(tmp_path / "r.json"))
    assert saved["n"] == scores["n"] == 1  # synthetic:4 keeps a quarter of the images for validation
    assert set(saved) == {"model", "bicubic", "per_image", "n", "args"}
    for name in ("model", "bicubic"):
        assert set(saved[name]) == {"psnr", "ssim", "sam", "ergas"}
        assert all(math.isfinite(v) for v in saved[name].values()), saved[name]
        assert all(len(v) == 1 for v in saved["per_image"][name].values())
    with pytest.raises(FileNotFoundError):
        evaluate.main(["--model_name", "never_trained", "--image_size", "32", "--magnification_factor", "2",
                       "--dataset_path", "synthetic:4"])


def test_trainer_without_the_flag_prints_no_metric_line(dev, tmp_path, monkeypatch, capsys):
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    T.main(_TRAIN + ["--model_name", "cli_plain"])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Val metrics" not in out
