"""No-data pixels without a GPU: the float64 oracle of tests/nodata_oracle.py against hand-worked cases, the argument refusals
of the four no-data entry points (csrc/nodata.hip, csrc/loss.hip, csrc/metrics.hip) through the library,
`feeds.load_sar_ndvi_folder(nodata=)`, the refusals of the trainers and the train state."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import nodata_oracle as NO

NAN = math.nan


# ---- the oracle against hand-worked cases ------------------------------------------------------------------------------------
def test_rule_by_hand():
    x = torch.tensor([[[0.5, NAN, 0.25, 0.25], [0.5, 0.1, 0.25, 0.3]]]).view(1, 2, 1, 4)  # 2 bands, 4 pixels
    assert NO.valid_mask(x).tolist() == [[[True, False, True, True]]]           # a NaN in one band is enough
    assert NO.valid_mask(x, NAN).tolist() == [[[True, False, True, True]]]      # NaN as the value: the NaN rule alone
    assert NO.valid_mask(x, 0.25).tolist() == [[[True, False, False, True]]]    # ALL bands equal the value (pixel 3: one band)
    assert NO.valid_mask(x, 0.5).tolist() == [[[False, False, True, True]]]
    # the compare is fp32's: 0.1 as a double is not the stored value, its fp32 rounding is
    y = torch.full((1, 1, 1, 1), 0.1)
    assert NO.valid_mask(y, 0.1).tolist() == [[[False]]]


def test_noise_target_by_hand():
    ah = torch.tensor([1.0, 0.64])  # t = 1: a = 0.8, b = 0.6 (as fp32 roots, widened)
    x0 = torch.tensor([0.5, NAN]).view(1, 1, 1, 2)
    eps = torch.tensor([2.0, -1.0]).view(1, 1, 1, 2)
    a, b = float(torch.sqrt(ah[1])), float(torch.sqrt(1.0 - ah[1]))
    for kind, want in (("eps", 2.0), ("v", a * 2.0 - b * 0.5), ("x0", 0.5)):
        x_t, target, valid = NO.noise_target(x0, eps, torch.tensor([1]), ah, kind, fill=0.25)
        assert valid.tolist() == [[[True, False]]]
        assert x_t.flatten().tolist() == [a * 0.5 + b * 2.0, a * 0.25 + b * -1.0]  # the no-data pixel: the noised fill
        assert target.flatten().tolist() == [want, 0.0]
    x_t, target, valid = NO.noise_target(x0, eps, torch.tensor([2]), ah, "eps")  # t outside the table
    assert torch.isnan(x_t).all() and torch.isnan(target).all() and not valid.any()


def test_masked_loss_by_hand():
    # B = 3, C = 2, two pixels: image 0 fully valid, image 1 one valid pixel, image 2 none
    pred = torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[1.0, NAN], [2.0, math.inf]], [[NAN, NAN], [1e30, 0.0]]]).view(3, 2, 1, 2)
    target = torch.zeros(3, 2, 1, 2)
    valid = torch.tensor([[True, True], [True, False], [False, False]]).view(3, 1, 2)
    w = torch.tensor([1.0, 3.0, 7.0], dtype=torch.float64)
    per_image, loss, grad, counts, Bv = NO.masked_loss(pred, target, valid, "MSE", w=w)
    assert counts.tolist() == [2, 1, 0] and Bv == 2
    assert per_image.tolist() == [(1 + 4 + 9 + 16) / 4, (1 + 4) / 2, 0.0]
    assert loss.item() == (1.0 * 7.5 + 3.0 * 2.5) / 2
    # grad = w_b 2 d / (Bv n_b): image 0: 2 d / 8, image 1: 6 d / 4 at its valid pixel, +0 elsewhere
    assert grad.flatten().tolist() == [0.25, 0.5, 0.75, 1.0, 1.5, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.signbit(grad).any()
    per_image, loss, grad, _, _ = NO.masked_loss(pred, target, valid, "MAE")
    assert per_image.tolist() == [2.5, 1.5, 0.0] and loss.item() == 2.0
    assert grad.flatten().tolist() == [0.125] * 4 + [0.25, 0.0, 0.25, 0.0] + [0.0] * 4
    per_image, loss, _, _, _ = NO.masked_loss(pred, target, valid, "Huber", delta=1.0)  # |d| >= 1 everywhere: |d| - 0.5
    assert per_image.tolist() == [2.0, 1.0, 0.0] and loss.item() == 1.5
    none = torch.zeros(3, 1, 2, dtype=torch.bool)
    per_image, loss, grad, counts, Bv = NO.masked_loss(pred, target, none, "MSE", w=w)
    assert Bv == 0 and loss.item() == 0.0 and per_image.tolist() == [0.0] * 3 and not grad.any()


def test_pointwise_and_quality_by_hand():
    # C = 2, four pixels; pixel 1 is NaN in band 0, pixel 3 holds the value 0.0 in both bands
    hr = torch.tensor([[0.5, NAN, 1.0, 0.0], [0.5, 0.3, 0.0, 0.0]]).view(1, 2, 1, 4)
    sr = torch.tensor([[0.5, 0.9, 0.0, NAN], [0.0, math.inf, 0.0, 0.7]]).view(1, 2, 1, 4)
    s = NO.pointwise_sums(sr, hr, 0.0)[0]
    assert s[:2].tolist() == [1.0, 0.25] and s[2:4].tolist() == [1.5, 0.5]  # sse and sum of hr per band, pixels 0 and 2
    # pixel 0: (0.5, 0) against (0.5, 0.5): 45 degrees; pixel 2: sr is the zero vector: no angle
    assert abs(s[4].item() - math.pi / 4) < 1e-15 and s[5].item() == 1.0 and s[6].item() == 2.0
    assert NO.pointwise_sums(sr, hr)[0, 6].item() == 3.0  # the NaN rule alone keeps pixel 3
    # the same four pixels in the first row of an 11 x 11 image whose other pixels hold the value: the sums do not change
    big_hr, big_sr = torch.zeros(1, 2, 11, 11), torch.full((1, 2, 11, 11), 0.4)
    big_hr[:, :, 0, :4], big_sr[:, :, 0, :4] = hr[:, :, 0], sr[:, :, 0]
    assert torch.equal(NO.pointwise_sums(big_sr, big_hr, 0.0)[0], s)
    q = NO.image_quality(big_sr, big_hr, 2, 0.0)
    assert q["valid_fraction"].tolist() == [2 / 121] and math.isnan(q["ssim"].item())  # (no window is whole)
    assert abs(q["psnr"].item() - 10 * math.log10(1 / (1.25 / 4))) < 1e-12
    assert abs(q["sam"].item() - 45.0) < 1e-12
    mse, mean = (0.5, 0.125), (0.75, 0.25)
    assert abs(q["ergas"].item() - 50 * math.sqrt((mse[0] / mean[0] ** 2 + mse[1] / mean[1] ** 2) / 2)) < 1e-12


def test_ssim_by_hand():
    g = torch.Generator().manual_seed(1)
    hr = torch.rand(3, 2, 12, 12, generator=g)
    sr = (hr + 0.05 * torch.randn(3, 2, 12, 12, generator=g)).clamp(0, 1)
    import metrics_oracle as MO
    full = NO.ssim(sr, hr)
    assert torch.equal(full[:, 1], torch.full((3,), 4.0, dtype=torch.float64))  # (12 - 10)^2 window positions
    assert torch.allclose(full[:, 0], MO.ssim(sr, hr), rtol=1e-13, atol=0)
    hr[1, 0, 0, 0] = NAN    # the corner pixel lies in the window at (0, 0) only
    hr[2, 1, 5, 5] = NAN    # a centre pixel lies in all four
    sr[1, :, 0, 0] = math.inf
    got = NO.ssim(sr, hr)
    assert got[:, 1].tolist() == [4.0, 3.0, 0.0] and math.isnan(got[2, 0].item()) and got[0, 0] == full[0, 0]
    # image 1: the mean of the other three positions, from the unmasked maps of the clean pair
    hr1, sr1 = hr[1:2].clone(), sr[1:2].clone()
    hr1[0, 0, 0, 0], sr1[0, :, 0, 0] = 0.3, 0.3
    hr1, sr1 = hr1.double(), sr1.double()
    B, Cc, H, W = sr1.shape
    w = MO.gaussian_window()[None, None]
    blur = lambda t: torch.nn.functional.conv2d(t.double().reshape(Cc, 1, H, W), w).reshape(Cc, 2, 2)  # noqa: E731
    mx, my = blur(sr1), blur(hr1)
    vx, vy, cxy = blur(sr1 * sr1) - mx * mx, blur(hr1 * hr1) - my * my, blur(sr1 * hr1) - mx * my
    q = ((2 * mx * my + 1e-4) * (2 * cxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
    want = (q.sum() - q[:, 0, 0].sum()) / (Cc * 3)
    assert abs(got[1, 0].item() - want.item()) < 1e-12


# ---- argument refusals through the library -------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    assert lib.drs_abi_version() == 8  # additions only
    buf, buf2 = C.create_string_buffer(1 << 16), C.create_string_buffer(1 << 16)
    p, q = C.cast(buf, C.c_void_p), C.cast(buf2, C.c_void_p)

    def noise(ptrs=(p, p, p, p, q, p, p), kind=0, n=1, Cc=3, hw=16, steps=10):
        x0, eps, t, ah, xt, target, valid = ptrs
        return lib.drs_noise_target_nodata(x0, eps, t, ah, steps, kind, NAN, 0.5, xt, target, valid, n, Cc, hw, None)
    for hole in range(7):
        assert noise(tuple(None if i == hole else v for i, v in enumerate((p, p, p, p, q, p, p)))) == 1
        assert b"null pointer" in lib.drs_last_error()
    assert noise((p, p, p, p, p, p, p)) == 1 and b"one buffer" in lib.drs_last_error()
    assert noise(kind=3) == 1 and b"kind" in lib.drs_last_error()
    for Cc in (0, 17, -1):
        assert noise(Cc=Cc) == 2 and b"C=" in lib.drs_last_error()
    assert noise(n=-1) == 2 and noise(hw=-1) == 2 and noise(steps=0) == 2
    assert noise(n=0) == 0 and noise(hw=0) == 0  # nothing to do, nothing launched

    def loss(ptrs=(p, p, p, p, p, p, p), t=None, table=None, bins=None, kind=0, delta=1.0, B=1, Cc=3, hw=16, T=0, nbins=0,
             history=0):
        pred, target, valid, per_image, counts, partials, out = ptrs
        return lib.drs_diffusion_loss_masked(pred, target, valid, t, B, Cc, hw, table, T, None, kind, delta, None, per_image,
                                             counts, partials, out, bins, nbins, history, 0, None, None)
    for hole in range(7):
        assert loss(tuple(None if i == hole else p for i in range(7))) == 1 and b"null pointer" in lib.drs_last_error()
    assert loss(kind=3) == 1 and b"unknown kind" in lib.drs_last_error()
    assert loss(kind=2, delta=0.0) == 1 and b"delta" in lib.drs_last_error()
    for kw in ({"B": 0}, {"B": 65536}, {"Cc": 0}, {"Cc": 17}, {"hw": 0}):
        assert loss(**kw) == 2, kw
    assert loss(table=p) == 1 and loss(table=p, t=p, T=0) == 1 and b"need t" in lib.drs_last_error()
    assert loss(bins=p, t=p, T=50, nbins=1, history=10) == 1 and b"nbins" in lib.drs_last_error()
    assert loss(bins=p, t=p, T=50, nbins=4, history=33) == 1 and b"history" in lib.drs_last_error()

    assert lib.drs_metrics_nodata_workspace_bytes(2, 3, 64, 72) >= lib.drs_metrics_workspace_bytes(2, 3, 64, 72) > 0
    assert lib.drs_metrics_nodata_workspace_bytes(1, 1, 11, 11) >= 2 * 8 + 121  # one SSIM sum, one count, the mask
    assert lib.drs_metrics_nodata_workspace_bytes(1, 17, 64, 64) == 0
    for fn in (lib.drs_metrics_pointwise_nodata, lib.drs_ssim_nodata):
        for hole in range(4):  # sr, hr, out, workspace
            ptrs = [None if i == hole else p for i in range(4)]
            assert fn(ptrs[0], ptrs[1], NAN, ptrs[2], 1, 3, 16, 16, 1, ptrs[3], 1 << 16, None) == 1
            assert b"null pointer" in lib.drs_last_error()
        assert fn(p, p, 0.0, p, 1, 17, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, 0.0, p, 1, 0, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, 0.0, p, 0, 3, 16, 16, 1, p, 1 << 16, None) == 2
        assert fn(p, p, 0.0, p, 1, 3, 16, 16, 1, p, 8, None) == 4
    assert lib.drs_ssim_nodata(p, p, NAN, p, 1, 3, 10, 16, 1, p, 1 << 16, None) == 2
    assert lib.drs_metrics_pointwise_nodata(p, p, NAN, p, 1, 3, 0, 16, 1, p, 1 << 16, None) == 2
    need = lib.drs_metrics_nodata_workspace_bytes(1, 3, 16, 16)
    assert need == (2 * 3 + 3) * 8 + 16 * 16  # one partial row of 2 C + 3 doubles (>= the 4 SSIM words), then the mask bytes
    assert lib.drs_ssim_nodata(p, p, NAN, p, 1, 3, 16, 16, 1, p, 4 * 8 + 16 * 16 - 1, None) == 4
    assert lib.drs_metrics_pointwise_nodata(p, p, NAN, p, 1, 3, 16, 16, 1, p, (2 * 3 + 3) * 8 - 1, None) == 4


def test_wrappers_have_no_cpu_path_and_check_the_rule():
    from diffusionremotesensing_amd import hip_ops, metrics
    from diffusionremotesensing_amd.losses import DiffusionLoss
    x = torch.rand(1, 3, 16, 16)
    for call in (lambda: metrics.psnr(x, x, nodata=True), lambda: metrics.ssim(x, x, nodata=0.0),
                 lambda: metrics.image_quality(x, x, 2, nodata="nan"), lambda: hip_ops.metrics_pointwise_nodata(x, x, True),
                 lambda: hip_ops.noise_target_nodata(x, x, torch.zeros(1, dtype=torch.int64), torch.ones(4), "eps"),
                 lambda: DiffusionLoss("MSE").loss_and_grad(x, x, valid=torch.ones(1, 1, 16, 16, dtype=torch.uint8))):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()
    assert math.isnan(hip_ops.nodata_rule(True)) and math.isnan(hip_ops.nodata_rule("nan")) and math.isnan(hip_ops.nodata_rule(NAN))
    assert hip_ops.nodata_rule(0) == 0.0 and hip_ops.nodata_rule(-9999.0) == -9999.0
    for bad in (None, False, "zero", math.inf):
        with pytest.raises(ValueError):
            hip_ops.nodata_rule(bad)


# ---- the folder loader ---------------------------------------------------------------------------------------------------------
def _write_pairs(root, data_format, sar, ndvi):
    for sub in ("sar", "opt"):
        os.makedirs(os.path.join(root, sub))
    for i, (s, n) in enumerate(zip(sar, ndvi)):
        for sub, img in (("sar", s), ("opt", n)):
            if data_format == "numpy":
                np.save(os.path.join(root, sub, f"{i:02d}.npy"), img.numpy())
            else:
                torch.save(img, os.path.join(root, sub, f"{i:02d}.pt"))


@pytest.mark.parametrize("data_format", ["numpy", "torch"])
def test_load_sar_ndvi_folder_nodata(tmp_path, data_format):
    from diffusionremotesensing_amd.feeds import load_sar_ndvi_folder, nodata_pixels
    g = torch.Generator().manual_seed(3)
    sar, ndvi = torch.rand(3, 2, 4, 5, generator=g) * 2 - 1, torch.rand(3, 2, 4, 5, generator=g) * 2 - 1
    V = -9999.0
    ndvi[0, :, 1, 2] = V           # the sentinel in all bands: no-data
    ndvi[0, 0, 2, 2] = V           # ... in one band only: data
    ndvi[1, 1, 0, 0] = NAN         # a NaN in one band: no-data
    sar[2, :, 3, 4] = V            # SAR no-data propagates to NDVI
    sar[2, 0, 0, 1] = NAN
    _write_pairs(str(tmp_path), data_format, sar, ndvi)
    plain_sar, plain_ndvi = load_sar_ndvi_folder(str(tmp_path), data_format)
    assert torch.equal(plain_sar.nan_to_num(7.0), sar.nan_to_num(7.0)) and torch.equal(plain_ndvi.nan_to_num(7.0), ndvi.nan_to_num(7.0))
    got_sar, got_ndvi = load_sar_ndvi_folder(str(tmp_path), data_format, nodata=V)
    want = torch.zeros(3, 4, 5, dtype=torch.bool)
    want[0, 1, 2] = want[1, 0, 0] = want[2, 3, 4] = want[2, 0, 1] = True
    assert torch.equal(torch.isnan(got_ndvi).all(dim=1), want) and torch.equal(torch.isnan(got_ndvi).any(dim=1), want)
    assert torch.equal(got_ndvi[~want[:, None].expand_as(ndvi)], ndvi[~want[:, None].expand_as(ndvi)])  # the rest untouched
    assert got_ndvi[0, 0, 2, 2] == V
    assert not torch.isnan(got_sar).any() and bool((got_sar[2, :, 3, 4] == 0).all()) and bool((got_sar[2, :, 0, 1] == 0).all())
    untouched = torch.ones(3, 4, 5, dtype=torch.bool)
    untouched[2, 3, 4] = untouched[2, 0, 1] = False
    assert torch.equal(got_sar[untouched[:, None].expand_as(sar)], sar[untouched[:, None].expand_as(sar)])
    # "nan": the NaN rule alone - the sentinel stays a value
    nan_sar, nan_ndvi = load_sar_ndvi_folder(str(tmp_path), data_format, nodata="nan")
    want_nan = torch.zeros(3, 4, 5, dtype=torch.bool)
    want_nan[1, 0, 0] = want_nan[2, 0, 1] = True
    assert torch.equal(torch.isnan(nan_ndvi).all(dim=1), want_nan) and bool((nan_ndvi[0, :, 1, 2] == V).all())
    assert bool((nan_sar[2, :, 3, 4] == V).all()) and bool((nan_sar[2, :, 0, 1] == 0).all())
    # the loader's rule is the oracle's
    assert torch.equal(~nodata_pixels(ndvi, V)[:, 0], NO.valid_mask(ndvi, V))
    # (v + 1) * 0.5, what the feed's kernels apply, keeps the marker
    assert torch.equal(torch.isnan((got_ndvi + 1) * 0.5), torch.isnan(got_ndvi))


# ---- the trainers' refusals and the train state ---------------------------------------------------------------------------------
def _stub(tmp_path, cls=None, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    cls = cls or Diffusion
    if cls is Diffusion:
        kw = {"magnification_factor": 2, "Degradation_type": "DownBlur", **kw}
    return cls("cosine", nn.Linear(3, 2), str(tmp_path / "run" / "snapshot.pt"), noise_steps=10, device="cpu", image_size=8, **kw)


def _train(d, loss="MSE", **kw):
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=[], val_loader=None, patience=5, loss=loss, verbose=False, **kw)
    return d


def test_trainer_refusals(tmp_path):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    from diffusionremotesensing_amd.losses import DiffusionLoss
    os.makedirs(tmp_path / "run")
    assert _stub(tmp_path).nodata is None and _stub(tmp_path, sar.Diffusion).nodata is None
    # the perceptual loss has no mask: refused before the VGG is built or a weight is touched
    for cls in (sr.Diffusion, sar.Diffusion):
        d = _stub(tmp_path, cls)
        d.nodata = True
        with pytest.raises(ValueError, match="MSE\\+Perceptual_noise cannot be combined with nodata"):
            _train(d, loss="MSE+Perceptual_noise")
    # BSRGAN sharpens its HR image
    d = _stub(tmp_path, Degradation_type="BSRGAN")
    d.nodata = 0.0
    with pytest.raises(ValueError, match="BSRGAN"):
        _train(d)
    with pytest.raises(ValueError, match="BSRGAN"):
        sr.nodata_u8_value(0, "BSRGAN")
    with pytest.raises(SystemExit):
        sr.parse_train_args(["--nodata", "0", "--Degradation_type", "BSRGAN"])
    with pytest.raises(SystemExit):
        sr.parse_train_args(["--nodata", "256"])
    assert sr.parse_train_args(["--nodata", "7"]).nodata == 7 and sr.parse_train_args([]).nodata is None
    assert sr.nodata_u8_value(7, "DownBlur") == float(np.float32(7) / np.float32(255)) and sr.nodata_u8_value(None, "BSRGAN") is None
    # the generation class refuses it
    d = _stub(tmp_path, gen.Diffusion)
    d.nodata = True
    with pytest.raises(ValueError, match="generation Diffusion does not take nodata"):
        _train(d)
    # a value that is no rule
    d = _stub(tmp_path)
    d.nodata = "zero"
    with pytest.raises(ValueError, match="nodata"):
        _train(d)
    # a run with nodata and a plain loss gets DiffusionLoss objects for both loops; a default run keeps torch's module
    d = _stub(tmp_path)
    d.nodata = True
    _train(d, loss="Huber")
    assert isinstance(d.train_state.loss_function, DiffusionLoss) and isinstance(d.train_state.val_loss_function, DiffusionLoss)
    assert d.train_state.loss_function.kind == "Huber" and d.train_state.objective is None
    os.remove(tmp_path / "run" / "snapshot.pt")
    d = _train(_stub(tmp_path))
    assert isinstance(d.train_state.loss_function, nn.MSELoss) and d.train_state.val_loss_function is None
    # the flags: 'nan' or a number on the SAR trainer, out of --help
    p = sar.train_main_parser()
    assert p.parse_args([]).nodata is None and p.parse_args(["--nodata", "nan"]).nodata == "nan"
    assert p.parse_args(["--nodata=-9999"]).nodata == -9999.0
    assert "--nodata" not in p.format_help()
    with pytest.raises(SystemExit):
        p.parse_args(["--nodata", "inf"])
    from diffusionremotesensing_amd import evaluate
    assert evaluate.cli_arg_parser("sar_to_ndvi").parse_args(["--nodata", "0.5"]).nodata == 0.5
    args = evaluate.cli_arg_parser("superres").parse_args(["--nodata", "7"])  # the stored byte, as on the trainer
    assert args.nodata == 7 and evaluate._evaluate_nodata(args, "superres") == float(np.float32(7) / np.float32(255))
    with pytest.raises(SystemExit):
        evaluate.cli_arg_parser("superres").parse_args(["--nodata", "0.5"])


def test_launcher_sets_nodata(monkeypatch):
    from diffusionremotesensing_amd import launcher
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    made = []

    class D:
        nodata = None

        def __init__(self, **kw):
            made.append(self)

        def train(self, **kw):
            self.seen_at_train = self.nodata
    args = sar.train_main_parser().parse_args([])
    args.snapshot_folder_path = "."
    launcher.train_model(args, D, nn.Linear(2, 2), "cpu", [], None)
    launcher.train_model(args, D, nn.Linear(2, 2), "cpu", [], None, nodata=True)
    assert [d.seen_at_train for d in made] == [None, True]


def test_train_state_mismatch_raises(tmp_path, monkeypatch):
    """train_state.pt carries `nodata` (as freeze_bn: only when set); a resume under another value is refused."""
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    os.makedirs(tmp_path / "run")
    path = str(tmp_path / "run" / "train_state.pt")
    written = {}
    real_save = torch.save
    monkeypatch.setattr(torch.cuda, "get_rng_state", lambda device=None: torch.zeros(1, dtype=torch.uint8))
    monkeypatch.setattr(torch, "save", lambda obj, p: (written.__setitem__(os.path.basename(str(p)), obj), real_save(obj, p)))
    for nodata, key in ((None, None), (True, "nan"), ("nan", "nan"), (0.1, float(np.float32(0.1))), (0, 0.0)):
        for f in ("snapshot.pt", "train_state.pt"):
            if os.path.exists(tmp_path / "run" / f):
                os.remove(tmp_path / "run" / f)
        d = _stub(tmp_path)
        d.nodata = nodata
        _train(d, save_train_state=True)
        assert written["train_state.pt"].get("NODATA") == key and ("NODATA" in written["train_state.pt"]) == (nodata is not None)
        assert Diffusion._nodata_key(nodata) == key
    # the file now on disk was written with nodata = 0
    base = {"RAW_MODEL_STATE": None, "LR_SCHEDULE": None, "OPTIMIZER_STATE": None}
    for saved, mine, words in ((0.0, None, "nodata=0.0, this run has nodata=None"), (0.0, True, "this run has nodata='nan'"),
                               (None, 0.5, "nodata=None, this run has nodata=0.5"), ("nan", 0.0, "nodata='nan'")):
        real_save({**base, **({} if saved is None else {"NODATA": saved})}, path)
        d = _stub(tmp_path)
        d.nodata = mine
        with pytest.raises(ValueError, match=words):
            _train(d, save_train_state=True)


def test_defaults_are_unchanged():
    """`nodata=None` is the old call: the new keywords are last and default to None."""
    import inspect
    from diffusionremotesensing_amd import feeds, metrics
    from diffusionremotesensing_amd.losses import DiffusionLoss
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    for fn in (metrics.image_quality, metrics.psnr, metrics.ssim, metrics.sam, metrics.ergas, feeds.load_sar_ndvi_folder,
               Diffusion.evaluate):
        assert list(inspect.signature(fn).parameters.items())[-1][0] == "nodata"
        assert inspect.signature(fn).parameters["nodata"].default is None
    for fn in (DiffusionLoss.loss_and_grad, DiffusionLoss.__call__):
        assert inspect.signature(fn).parameters["valid"].default is None
