"""Colour correction on the GPU (csrc/colorfix.hip through diffusionremotesensing_amd.colorfix) against the float64 oracle of
tests/colorfix_oracle.py, and its use by the tiler and by `Diffusion.evaluate`."""
import pytest
import torch

import colorfix_oracle as CO
from conftest import replay_noise_source, replay_tile_noise

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# Derived, not measured.  Wavelet: the weights are powers of two, a level costs 4 roundings in the separable form (8 as a
# 9-tap sum), each at most 2^-24 * 2 M with M = max(|sr|, |guide|); the blurs are convex combinations and amplify nothing;
# with the subtraction and the final add that is at most 45 (85) units of 2^-24 M.  AdaIN: three fp32 roundings (a, b, the
# fused multiply-add) on terms of the sizes |a sr|, |b|, |want|, and a factor 8 for the statistics.
WAVELET_UNITS, ADAIN_UNITS = 128, 8

SHAPES = [(1, 1, 1, 1),      # every tap clamps to one pixel
          (1, 1, 5, 7),      # smaller than every dilation >= 8: both borders clamp at once
          (2, 3, 33, 47),    # odd, H * W % 4 != 0, one side about the halo
          (1, 16, 64, 72),   # 16 bands
          (1, 3, 130, 200)]  # several tiles both ways, interior tiles with a full halo
LEVELS = (1, 3, 5)
_ids = {"ids": lambda s: "x".join(map(str, s))}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _noise(shape, seed):
    """Uniform in [-0.2, 1.2]."""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 1.4 - 0.2


def _wavelet_units(got, want, sr, guide):
    """The worst error in units of 2^-24 M."""
    M = max(sr.abs().max().item(), guide.abs().max().item())
    return ((got.double() - want).abs().max() / (EPS * M)).item()


def _adain_units(got, sr, guide):
    """The worst error in units of 2^-24 (|a sr| + |b| + |want|), per element, with the oracle's coefficients."""
    want = CO.adain(sr, guide)
    a, b = CO.adain_coefficients(sr, guide)
    scale = EPS * ((a * sr.double()).abs() + b.abs() + want.abs())
    return ((got.double() - want).abs() / scale).max().item()


@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_wavelet_vs_float64_oracle(dev, shape):
    """Levels 1, 3 and 5 on uniform noise, on guide = sr + 0.25 (the weights sum to 1: the result is sr + 0.25) and on guide ==
    sr (the result is sr bit for bit); |got - want| <= 128 * 2^-24 * M.
    Measured on MI355X, worst over the levels, units of 2^-24 M, noise / shifted, (1,1,1,1) / (1,1,5,7) / (2,3,33,47) /
    (1,16,64,72) / (1,3,130,200): 0.00 / 0.95 / 1.34 / 2.17 / 1.69 and 0.54 / 0.70 / 0.80 / 0.81 / 0.85."""
    from diffusionremotesensing_amd import hip_ops
    sr, guide = _noise(shape, 11 + sum(shape)), _noise(shape, 12 + sum(shape))
    shifted = sr + 0.25
    for levels in LEVELS:
        got = hip_ops.colorfix_wavelet(sr.to(dev), guide.to(dev), levels).cpu()
        assert got.shape == sr.shape and got.dtype == torch.float32
        u = _wavelet_units(got, CO.wavelet(sr, guide, levels), sr, guide)
        print(f"wavelet {shape} L={levels}: noise {u:.2f} units of 2^-24 M")
        assert u <= WAVELET_UNITS, (shape, levels, u)
        got = hip_ops.colorfix_wavelet(sr.to(dev), shifted.to(dev), levels).cpu()
        u = max(_wavelet_units(got, CO.wavelet(sr, shifted, levels), sr, shifted),
                _wavelet_units(got, sr.double() + 0.25, sr, shifted))
        print(f"wavelet {shape} L={levels}: shifted {u:.2f} units")
        assert u <= WAVELET_UNITS, (shape, levels, u)
        same = hip_ops.colorfix_wavelet(sr.to(dev), sr.clone().to(dev), levels).cpu()
        assert torch.equal(same, sr), (shape, levels)
    # a wrong level count is far outside the bound
    if shape[2] >= 33:
        assert _wavelet_units(hip_ops.colorfix_wavelet(sr.to(dev), guide.to(dev), 4).cpu(), CO.wavelet(sr, guide, 5), sr, guide) > 1e4


@pytest.mark.parametrize("shape", SHAPES[1:], **_ids)
def test_adain_vs_float64_oracle(dev, shape):
    """Uniform noise, and flat bright terrain (0.95 +- 0.002) against a guide of deviation 0.1 (a = 27 with the 1e-5 under both roots), where a variance lost
    to cancellation would show: |got - want| <= 8 * 2^-24 * (|a sr| + |b| + |want|) per element.
    Measured on MI355X, units of that scale, noise / bright_flat, (1,1,5,7) / (2,3,33,47) / (1,16,64,72) / (1,3,130,200):
    0.51 / 0.64 / 0.97 / 0.76 and 0.06 / 0.48 / 0.50 / 0.17."""
    from diffusionremotesensing_amd import hip_ops
    g = torch.Generator().manual_seed(21 + sum(shape))
    cases = {"noise": (_noise(shape, 13 + sum(shape)), _noise(shape, 14 + sum(shape))),
             "bright_flat": (0.95 + 0.002 * torch.randn(shape, generator=g), 0.4 + 0.1 * torch.randn(shape, generator=g))}
    for name, (sr, guide) in cases.items():
        got = hip_ops.colorfix_adain(sr.to(dev), guide.to(dev)).cpu()
        assert got.shape == sr.shape and got.dtype == torch.float32
        u = _adain_units(got, sr, guide)
        print(f"adain {shape} {name}: {u:.2f} units of 2^-24 (|a sr| + |b| + |want|)")
        assert u <= ADAIN_UNITS, (shape, name, u)
    a, _ = CO.adain_coefficients(*cases["bright_flat"])
    assert shape[2] * shape[3] < 1000 or a.min().item() > 15  # (sqrt(1e-2 + 1e-5) / sqrt(4e-6 + 1e-5) = 27)


def test_impulse_response(dev):
    """sr = 0 and a guide that is one at a corner, at an edge midpoint and at the centre of 130 x 200, L = 5: the response is
    exactly zero further than 31 pixels from the impulse and within the bound of the oracle."""
    from diffusionremotesensing_amd import hip_ops
    H, W = 130, 200
    sr = torch.zeros((1, 3, H, W))
    guide = torch.zeros((1, 3, H, W))
    at = [(0, 0), (0, W // 2), (H // 2, W // 2)]
    for c, (y, x) in enumerate(at):
        guide[0, c, y, x] = 1.0
    got = hip_ops.colorfix_wavelet(sr.to(dev), guide.to(dev), 5).cpu()
    assert _wavelet_units(got, CO.wavelet(sr, guide, 5), sr, guide) <= WAVELET_UNITS
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for c, (y, x) in enumerate(at):
        far = ((yy - y).abs() > 31) | ((xx - x).abs() > 31)
        assert (got[0, c][far] == 0).all() and got[0, c][~far].min().item() >= 0 and got[0, c, y, x].item() > 0
    assert got[0, 2].double().sum().item() == pytest.approx(1.0, abs=1e-5)  # (away from the replicating borders: unit mass)


def test_repeatable_unaligned_and_refusals(dev):
    """Two calls write the same bits, for both methods; a view whose planes are not 16-byte aligned takes the element-wise
    paths and agrees with the oracle; non-contiguous and CPU tensors are refused; H W = 1 has no variance."""
    from diffusionremotesensing_amd import color_fix, hip_ops
    shape = (2, 3, 70, 132)
    sr, guide = _noise(shape, 31).to(dev), _noise(shape, 32).to(dev)
    for fn in (lambda a, b: hip_ops.colorfix_wavelet(a, b, 5), hip_ops.colorfix_adain):
        assert torch.equal(fn(sr, guide), fn(sr, guide))
    small = (2, 3, 16, 16)
    big_s, big_g = _noise((2, 3, 16, 17), 33), _noise((2, 3, 16, 17), 34)
    off_s, off_g = (t.to(dev).flatten()[1:1 + 2 * 3 * 16 * 16].view(small) for t in (big_s, big_g))
    assert off_s.data_ptr() % 16 != 0 and off_s.is_contiguous()
    assert _wavelet_units(hip_ops.colorfix_wavelet(off_s, off_g, 3).cpu(), CO.wavelet(off_s.cpu(), off_g.cpu(), 3), off_s.cpu(),
                          off_g.cpu()) <= WAVELET_UNITS
    assert _adain_units(hip_ops.colorfix_adain(off_s, off_g).cpu(), off_s.cpu(), off_g.cpu()) <= ADAIN_UNITS
    for fn in (hip_ops.colorfix_wavelet, hip_ops.colorfix_adain):
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(sr.transpose(2, 3), guide.transpose(2, 3))
        with pytest.raises(RuntimeError, match="contiguous"):
            fn(sr, torch.zeros(shape[:3] + (2 * shape[3],), device=dev)[..., ::2])
        with pytest.raises(RuntimeError, match="ROCm"):
            fn(sr.cpu(), guide.cpu())
        with pytest.raises(RuntimeError, match="same"):
            fn(sr, guide[:1])
    with pytest.raises(RuntimeError, match="status 2"):
        hip_ops.colorfix_adain(sr[:1, :1, :1, :1].contiguous(), guide[:1, :1, :1, :1].contiguous())
    with pytest.raises(RuntimeError, match="status 2"):
        hip_ops.colorfix_wavelet(sr, guide, 6)
    # the public function: lr is up-sampled with the bicubic kernel, a (C, H, W) scene comes back as one
    lr = _noise((2, 3, 35, 66), 35).to(dev)
    via_lr = color_fix(sr, lr, magnification_factor=2)
    assert torch.equal(via_lr, hip_ops.colorfix_wavelet(sr, hip_ops.bicubic_upsample(lr, 2), 5))
    assert torch.equal(color_fix(sr[0], lr[0], magnification_factor=2, levels=3),
                       hip_ops.colorfix_wavelet(sr[:1], hip_ops.bicubic_upsample(lr[:1], 2), 3)[0])
    assert torch.equal(color_fix(sr, guide=guide, method="adain"), hip_ops.colorfix_adain(sr, guide))


# ---------------------------------------------------------------------------------------------
# tiler and Diffusion.evaluate
# ---------------------------------------------------------------------------------------------
def _superres(dev, sd, T, image_size=64):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    return m, Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                        image_size=image_size, Degradation_type="DownBlur")


@pytest.mark.parametrize("mode", ["final", "per_step"])
def test_tiler_corrects_the_finished_scene_once(dev, seeded_sd, mode):
    """LR scene 48 x 40 whose bands differ in brightness, patch 32, stride 16, x2, T = 6.  `color_fix=None` is the call without
    the argument, bit for bit; with "wavelet" the result is clamp(color_fix(plain result, lr=img_lr)) bit for bit - the whole
    scene corrected once - and its per-band means lie closer to the up-sampled LR image's than the plain result's do."""
    from diffusionremotesensing_amd import color_fix, hip_ops, synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T = 6
    m, d = _superres(dev, seeded_sd, T)
    img = (0.25 * synthetic.tensor_uniform("colorfix.img", (1, 3, 48, 40)) + torch.tensor([0.05, 0.25, 0.65]).view(1, 3, 1, 1)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)

    def run(**kw):
        src = (replay_tile_noise(77, len(tiler.patches_lr), T, (1, 3, 64, 64)) if mode == "final" else replay_noise_source(77))
        out = tiler.aggregation_sampling(noise_source=src, aggregation=mode, **kw)
        m.eval()
        return out
    plain = run()
    assert plain.shape == (1, 3, 96, 80) and torch.equal(plain, run(color_fix=None))
    fixed = run(color_fix="wavelet")
    assert torch.equal(fixed, torch.clamp(color_fix(plain, lr=img, magnification_factor=2), 0, 1))
    assert not torch.equal(fixed, plain) and fixed.min().item() >= 0 and fixed.max().item() <= 1
    assert torch.equal(run(color_fix="wavelet", color_fix_levels=2),
                       torch.clamp(color_fix(plain, lr=img, magnification_factor=2, levels=2), 0, 1))
    assert torch.equal(run(color_fix="adain"), torch.clamp(color_fix(plain, lr=img, magnification_factor=2, method="adain"), 0, 1))
    want = hip_ops.bicubic_upsample(img, 2).mean(dim=(0, 2, 3))
    before, after = (plain.mean(dim=(0, 2, 3)) - want).abs(), (fixed.mean(dim=(0, 2, 3)) - want).abs()
    print(f"tiler [{mode}]: per-band |mean - guide mean| {before.tolist()} -> {after.tolist()}")
    assert (after < before).all()


def test_evaluate_adds_model_fixed_and_samples_once(dev, seeded_sd):
    """Two batches of two synthetic images, T = 8, DDIM S = 4: "model_fixed" appears next to "model" and "bicubic", "model" is
    the run without color_fix under the same noise, every batch is sampled once, and "model_fixed" scores the corrected,
    clamped sample of that one call."""
    from diffusionremotesensing_amd import color_fix, metrics, synthetic
    m, d = _superres(dev, seeded_sd, 8)
    hr = synthetic.tensor_uniform("metrics.hr", (4, 3, 64, 64))
    lr = synthetic.tensor_uniform("metrics.lr", (4, 3, 32, 32))
    loader = [(lr[:2], hr[:2]), (lr[2:], hr[2:])]
    plain = d.evaluate(m, loader, sampling_steps=4, noise_source=replay_noise_source(31))
    assert set(plain) == {"model", "bicubic", "per_image", "n"}
    calls, samples, inner = [], [], d.sample

    def counting(*args, **kw):
        calls.append(args[0])
        samples.append(inner(*args, **kw))
        return samples[-1]
    d.sample = counting
    res = d.evaluate(m, loader, sampling_steps=4, noise_source=replay_noise_source(31), color_fix="wavelet")
    assert calls == [2, 2]
    assert set(res) == {"model", "bicubic", "model_fixed", "per_image", "n"} and res["n"] == 4
    assert set(res["per_image"]) == {"model", "bicubic", "model_fixed"}
    assert res["model"] == plain["model"] and res["per_image"]["model"] == plain["per_image"]["model"]
    assert res["bicubic"] == plain["bicubic"]
    fixed = color_fix(torch.cat(samples).clamp(0, 1), lr.to(dev), magnification_factor=2)
    want = metrics.image_quality(fixed, hr.to(dev), 2)
    assert set(res["model_fixed"]) == {"psnr", "ssim", "sam", "ergas"}
    for k, v in want.items():
        assert res["per_image"]["model_fixed"][k] == v.tolist(), k
    assert res["per_image"]["model_fixed"]["psnr"] != res["per_image"]["model"]["psnr"]
    three = d.evaluate(m, loader, n_images=3, sampling_steps=4, noise_source=replay_noise_source(31), color_fix="adain",
                       baseline=False)
    assert calls == [2, 2, 2, 1] and set(three) == {"model", "model_fixed", "per_image", "n"} and three["n"] == 3
