"""Image-quality metrics without a GPU: the float64 oracle against closed forms, the argument validation of the new C-ABI
entry points, and the command lines."""
import ctypes as C
import math

import pytest
import torch

import metrics_oracle as M


def _const(a, shape=(2, 3, 16, 20)):
    return torch.full(shape, a, dtype=torch.float64)


@pytest.mark.parametrize("a,b", [(0.3, 0.7), (0.95, 0.9), (0.0, 1.0), (0.5, 0.5)])
def test_oracle_constant_images(a, b):
    """Constant images a and b: every window has means a, b and no variance, so SSIM = (2ab + C1) / (a^2 + b^2 + C1) (the
    structure term is C2 / C2), and PSNR = -20 log10 |a - b|."""
    x, y = _const(a), _const(b)
    c1 = 0.01 ** 2
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    assert torch.allclose(M.ssim(x, y), torch.full((2,), want, dtype=torch.float64), rtol=0, atol=1e-12)
    if a != b:
        assert torch.allclose(M.psnr(x, y), torch.full((2,), -20 * math.log10(abs(a - b)), dtype=torch.float64), atol=1e-10)
    else:
        assert torch.isinf(M.psnr(x, y)).all() and (M.psnr(x, y) > 0).all()


def test_oracle_window_is_normalised_and_separable():
    w = M.gaussian_window()
    assert w.shape == (11, 11) and abs(w.sum().item() - 1) < 1e-15
    assert torch.allclose(w, w.t()) and torch.allclose(w[5] / w[5, 5], w[:, 5] / w[5, 5])
    assert abs(w[5, 4].item() / w[5, 5].item() - math.exp(-1 / 4.5)) < 1e-15


def test_oracle_spectral_angle():
    g = torch.Generator().manual_seed(3)
    hr = torch.rand((2, 5, 12, 13), generator=g, dtype=torch.float64) * 0.5 + 0.1
    assert M.sam(0.37 * hr, hr).abs().max().item() < 1e-6  # sr = k hr: parallel spectra (float64 rounding only)
    assert M.sam(hr, hr).abs().max().item() == 0.0
    u = torch.tensor([0.3, 0.0, 0.4, 0.0]).view(1, 4, 1, 1).expand(1, 4, 11, 12)
    v = torch.tensor([0.0, 0.8, 0.0, 0.1]).view(1, 4, 1, 1).expand(1, 4, 11, 12)
    assert abs(M.sam(u, v).item() - 90.0) < 1e-12  # two fixed orthogonal spectra
    w = torch.tensor([1.0, 1.0, 0.0, 0.0]).view(1, 4, 1, 1).expand(1, 4, 11, 12) * 0.5
    x = torch.tensor([1.0, 0.0, 0.0, 0.0]).view(1, 4, 1, 1).expand(1, 4, 11, 12) * 0.9
    assert abs(M.sam(w, x).item() - 45.0) < 1e-12


def test_oracle_zero_pixels_are_left_out_of_the_angle():
    u = torch.tensor([0.5, 0.0]).view(1, 2, 1, 1).expand(1, 2, 11, 12).clone()
    v = torch.tensor([0.0, 0.5]).view(1, 2, 1, 1).expand(1, 2, 11, 12).clone()
    u[0, :, :5] = 0  # no vector in sr: these pixels have no angle
    v[0, :, 8:] = -3  # clamped to zero: none in hr either
    assert abs(M.sam(u, v).item() - 90.0) < 1e-12
    assert math.isnan(M.sam(torch.zeros_like(u), v).item())
    assert abs(M.sam(u, v, clamp=False)[0].item() - (3 * 90.0 + 3 * 135.0) / 6) < 1e-12


@pytest.mark.parametrize("r,mag", [(0.01, 2), (0.05, 4)])
def test_oracle_ergas_of_a_uniform_relative_error(r, mag):
    """sr = (1 + r) hr with hr constant per band: MSE_c = r^2 mean_c^2 in every band, so ERGAS = 100 r / mag."""
    means = torch.tensor([0.2, 0.5, 0.8], dtype=torch.float64).view(1, 3, 1, 1)
    hr = means.expand(2, 3, 11, 14)
    assert torch.allclose(M.ergas((1 + r) * hr, hr, mag), torch.full((2,), 100 * r / mag, dtype=torch.float64), rtol=1e-12)
    dark = hr.clone()
    dark[1, 2] = 0
    e = M.ergas(dark + 0.1, dark, mag)
    assert math.isfinite(e[0].item()) and math.isinf(e[1].item())  # a band whose truth has mean 0


def test_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    assert lib.drs_metrics_workspace_bytes(2, 3, 64, 72) > 0
    assert lib.drs_metrics_workspace_bytes(1, 1, 11, 11) > 0
    assert lib.drs_metrics_workspace_bytes(1, 17, 64, 64) == 0
    for fn in (lib.drs_metrics_pointwise, lib.drs_ssim):
        for hole in range(4):  # sr, hr, out, workspace
            ptrs = [None if i == hole else p for i in range(4)]
            assert fn(ptrs[0], ptrs[1], ptrs[2], 1, 3, 16, 16, 1, ptrs[3], 1 << 16, None) == 1
            assert b"null pointer" in lib.drs_last_error()
        assert fn(p, p, p, 1, 17, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, p, 1, 0, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, p, 0, 3, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, p, 1, 3, 16, 16, 1, p, 8, None) == 4
    assert lib.drs_ssim(p, p, p, 1, 3, 10, 16, 1, p, 1 << 16, None) == 2
    assert lib.drs_ssim(p, p, p, 1, 3, 16, 10, 1, p, 1 << 16, None) == 2
    assert lib.drs_metrics_pointwise(p, p, p, 1, 3, 0, 16, 1, p, 1 << 16, None) == 2


def test_metrics_have_no_cpu_path():
    from diffusionremotesensing_amd import hip_ops, metrics
    x = torch.rand(1, 3, 16, 16)
    for call in (lambda: metrics.psnr(x, x), lambda: metrics.ssim(x, x), lambda: metrics.ergas(x, x, 2),
                 lambda: metrics.image_quality(x, x, 2), lambda: hip_ops.metrics_pointwise(x, x)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()
    with pytest.raises(ValueError, match="2 bands"):
        metrics.sam(torch.rand(1, 1, 16, 16), torch.rand(1, 1, 16, 16))


def test_evaluate_parser_takes_the_trainer_flags():
    from diffusionremotesensing_amd import evaluate
    a = evaluate.evaluate_arg_parser().parse_args(
        ["--image_size", "64", "--model_name", "m", "--magnification_factor", "2", "--inp_out_channels", "13",
         "--noise_steps", "50", "--dataset_path", "synthetic:8", "--Degradation_type", "DownBlur", "--Blur_radius", "0.5",
         "--snapshot_name", "s.pt", "--batch_size", "4", "--sampling_steps", "10", "--eta", "0.5", "--n_images", "3",
         "--out", "r.json"])
    assert (a.image_size, a.inp_out_channels, a.sampling_steps, a.eta, a.n_images, a.out) == (64, 13, 10, 0.5, 3, "r.json")
    d = evaluate.evaluate_arg_parser().parse_args(["--model_name", "m"])
    assert d.n_images is None and d.out == "results.json" and d.sampling_steps is None
    with pytest.raises(SystemExit):
        evaluate.main(["--model_name", "m", "--image_size", "64", "--magnification_factor", "2", "--multiple_gpus", "True"])


def test_eval_metrics_flag_is_off_by_default_and_rejected_with_multiple_gpus(capsys):
    from diffusionremotesensing_amd.train_diffusion_superres import parse_train_args
    base = ["--image_size", "64", "--model_name", "m", "--loss", "MSE", "--magnification_factor", "2"]
    assert parse_train_args(base).eval_metrics == 0
    assert parse_train_args(base + ["--eval_metrics", "4", "--sampling_steps", "10"]).eval_metrics == 4
    with pytest.raises(SystemExit):
        parse_train_args(base + ["--eval_metrics", "4", "--multiple_gpus", "True"])
    assert "--multiple_gpus" in capsys.readouterr().err
    assert parse_train_args(base + ["--multiple_gpus", "True"]).multiple_gpus is True


def test_score_formats():
    from diffusionremotesensing_amd.evaluate import format_table
    from diffusionremotesensing_amd.train_diffusion_superres import format_scores
    scores = {"model": {"psnr": 23.456789, "ssim": 0.87654321, "sam": 1.23456, "ergas": 12.34567},
              "bicubic": {"psnr": 20.0, "ssim": 0.5, "sam": 2.0, "ergas": 0.0123456}, "n": 4}
    line = format_scores(scores)
    assert line == ("model PSNR 23.46 dB SSIM 0.8765 SAM 1.235 deg ERGAS 12.35 | "
                    "bicubic PSNR 20.00 dB SSIM 0.5000 SAM 2.000 deg ERGAS 0.01235")
    table = format_table(scores).splitlines()
    assert len(table) == 3 and table[1].split() == ["model", "23.46", "dB", "0.8765", "1.235", "deg", "12.35"]
    assert format_scores({"model": {"psnr": 10.0, "ssim": 0.1}}) == "model PSNR 10.00 dB SSIM 0.1000"
