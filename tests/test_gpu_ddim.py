"""DDIM sampling on the GPU (drs_ddim_step and `Diffusion.sample(..., sampling_steps=S, eta=eta)` of the three models and the
tiler) against the float64 DDIM oracle of tests/ddim_oracle.py, which drives the CPU oracle UNets with the same noise draws."""
import os

import pytest
import torch

import ddim_oracle as O
from conftest import rel_errors, replay_noise_source
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U

pytestmark = pytest.mark.gpu

IMPLS = [i for i in os.environ.get("DRS_TEST_IMPLS", "direct,mfma_f32,mfma_bf16x3").split(",") if i]
_ORACLE = {}  # oracle chains are computed once per case and shared by the impls


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, seeded_sd):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    return m.to(dev).eval()


def _oracle(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _psnr_clamped(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).mean().item()
    return float("inf") if mse == 0 else -10 * torch.log10(torch.tensor(mse)).item()


# rel-L2 and PSNR (dB, on the [0,1]-clamped images) bounds per chain family: (exact fp32, split bf16), ~10x the rel-L2 (and
# 20 dB under the PSNR) measured on MI355X for the worst case of the family (rel-L2, fp32 / split bf16: superres 64^2 1.2e-6 /
# 2.1e-5, 99 / 78 dB; T = 1500 2.8e-7 / 3.6e-7, 138 / 110 dB; SAR 5.5e-7 / 6.5e-6, 114 / 92 dB; generation 1.6e-6 / 2.0e-5,
# 104 / 83 dB)
BOUNDS = {"superres": ((1.2e-5, 79.0), (2.2e-4, 57.0)), "long": ((3e-6, 118.0), (4e-6, 90.0)),
          "sar": ((6e-6, 93.0), (7e-5, 72.0)), "generation": ((1.6e-5, 83.0), (2e-4, 62.0))}


def _check_chain(family, what, impl, got, want):
    e_max, e_l2 = rel_errors(got, want)
    psnr = _psnr_clamped(got, want)
    if impl in ("direct", "mfma_f32"):
        l2_bound, psnr_bound = BOUNDS[family][0]
    elif impl == "mfma_bf16x3":
        l2_bound, psnr_bound = BOUNDS[family][1]
    else:  # opt-in mfma_f16
        l2_bound, psnr_bound = 5e-3, 40.0
    print(f"ddim {what} [{impl}]: max-rel {e_max:.3e} rel-L2 {e_l2:.3e} PSNR {psnr:.1f} dB")
    assert torch.isfinite(got).all()
    assert e_l2 <= l2_bound and psnr >= psnr_bound, (what, impl, e_l2, psnr)


# ---------------------------------------------------------------------------------------------
# the step kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_ddim_step_kernel_vs_float64_oracle(dev, kind):
    """drs_ddim_step against the float64 step: error / max(|A x| + |B eps| + |sigma z|) <= 1e-6, bit-stable over calls."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule(kind, 1500)
    ah_d = ah.to(dev)
    g = torch.Generator().manual_seed(11)
    x, ec, eu, z = (torch.randn((2, 3, 16, 20), generator=g) for _ in range(4))
    xd, ecd, eud, zd = (a.to(dev) for a in (x, ec, eu, z))
    worst = 0.0
    for t, tp in ((49, 42), (1499, 1469), (7, 1), (1, 0), (1499, 0)):
        for eta in (0.0, 0.5, 1.0):
            for w in (None, 0.3, 3.0):
                noise = None if eta == 0 else z
                eps64 = ec.double() if w is None else O.lerp64(eu, ec, w)
                A, B, sigma = O.coefficients(t, tp, eta, ah)
                want = O.step(x, eps64, noise, t, tp, eta, ah)
                scale = (A * x.double()).abs() + (B * eps64).abs()
                if sigma > 0:
                    scale = scale + (sigma * z.double()).abs()
                outs = []
                for _ in range(2):
                    outs.append(hip_ops.ddim_step_(xd.clone(), ecd, zd if noise is not None else None, t, tp, eta, ah_d,
                                                   eps_uncond=eud if w is not None else None,
                                                   cfg_scale=w if w is not None else 0.0).cpu())
                assert torch.equal(outs[0], outs[1]), (t, tp, eta, w)
                err = ((outs[0].double() - want).abs().max() / scale.max()).item()
                worst = max(worst, err)
                assert err <= 1e-6, (kind, t, tp, eta, w, err, A, B, sigma)
    print(f"ddim step kernel [{kind}]: worst normalised error {worst:.3e}")


def test_ddim_step_rejects_bad_tensors(dev):
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 50)
    x = torch.zeros((2, 3, 8, 8), device=dev)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.ddim_step_(x, torch.zeros((2, 3, 8, 7), device=dev), None, 10, 5, 0.0, ah.to(dev))
    with pytest.raises(RuntimeError, match="noise"):
        hip_ops.ddim_step_(x, torch.zeros_like(x), None, 10, 5, 0.5, ah.to(dev))
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.ddim_step_(x, torch.zeros_like(x), None, 10, 5, 0.0, ah)  # the table must live on the device


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("S,eta", [(7, 0.0), (7, 1.0), (49, 0.0), (49, 1.0)])
def test_superres_ddim_chain_vs_oracle(dev, model, seeded_sd, impl, S, eta):
    """n = 2, 64x64 (LR 32x32, x2), cosine T = 50; S = 49 is the ancestral chain's timestep set."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    model.hip_engine().set_impl(impl)
    d = Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, magnification_factor=2,
                  image_size=64, Degradation_type="DownBlur")
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    x = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), sampling_steps=S, eta=eta).cpu()
    assert model.training  # same side effect as the ancestral sampler
    model.eval()
    _, ah, _ = D.schedule("cosine", 50)
    want = _oracle(("sr", S, eta), lambda: O.sample_superres(U.OracleUNet(seeded_sd), 2, lr1, 50, ah, 2, 64, S, eta,
                                                             replay_noise_source(505)))
    _check_chain("superres", f"superres S={S} eta={eta}", impl, x, want)


@pytest.mark.parametrize("impl", IMPLS)
def test_superres_ddim_long_schedule_vs_oracle(dev, seeded_sd, impl):
    """configs[1]'s schedule (cosine T = 1500) in 50 DDIM steps at 32x32, n = 2: jumps of 30 timesteps from ah ~ 1e-6,
    where the step coefficients reach ~1e2 - 1e3.  `output` damped as in the long ancestral chain test."""
    from conftest import longchain_state_dict
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    sd = longchain_state_dict(seeded_sd)
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=2,
                  image_size=32, Degradation_type="DownBlur")
    lr1 = synthetic.tensor_uniform("ddim.long.lr", (3, 16, 16))
    x = d.sample(2, m, lr1, input_channels=3, noise_source=replay_noise_source(1500), sampling_steps=50, eta=0.0).cpu()
    _, ah, _ = D.schedule("cosine", 1500)
    want = _oracle("long", lambda: O.sample_superres(U.OracleUNet(sd), 2, lr1, 1500, ah, 2, 32, 50, 0.0,
                                                     replay_noise_source(1500)))
    _check_chain("long", "superres T=1500 S=50", impl, x, want)


@pytest.mark.parametrize("impl", IMPLS)
def test_sar_ddim_chain_vs_oracle(dev, seeded_sd_sar, impl):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(seeded_sd_sar)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=30, device=dev, image_size=64)
    sar1 = synthetic.tensor_uniform("ddim.sar", (2, 64, 64))
    x = d.sample(2, m, sar1, NDVI_channels=1, noise_source=replay_noise_source(303), sampling_steps=10, eta=0.5).cpu()
    _, ah, _ = D.schedule("cosine", 30)
    want = _oracle("sar", lambda: O.sample_sar(U.OracleUNetSAR(seeded_sd_sar), 2, sar1, 30, ah, 64, 10, 0.5,
                                               replay_noise_source(303)))
    _check_chain("sar", "sar T=30 S=10 eta=0.5", impl, x, want)


@pytest.mark.parametrize("impl", IMPLS)
def test_generation_guided_ddim_chain_vs_oracle(dev, seeded_sd_gen, impl):
    """Classifier-free guidance 3: one 2n-row forward per step into the CFG form of drs_ddim_step."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=20, device=dev, image_size=32)
    cls = torch.tensor([2, 5])
    x = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(202),
                 sampling_steps=6, eta=1.0).cpu()
    _, ah, _ = D.schedule("cosine", 20)
    want = _oracle("gen", lambda: O.sample_generation(U.OracleUNetGeneration(seeded_sd_gen), 2, cls, 3, 20, ah, 32, 6, 1.0,
                                                      replay_noise_source(202)))
    _check_chain("generation", "generation cfg=3 T=20 S=6 eta=1", impl, x, want)


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
def test_aggregation_ddim_vs_oracle(dev, seeded_sd, impl):
    """A two-tile scene through split_aggregation_sampling with sampling_steps=5, eta=0 against per-tile oracle DDIM chains
    blended like the reference."""
    from conftest import replay_tile_noise
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from oracle import aggregation_oracle as A
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    T = 50
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                  image_size=64, Degradation_type="DownBlur")
    img = synthetic.tensor_uniform("ddim.agg.img", (1, 3, 32, 48))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(32, 48, 32, 16, 2)
    assert len(infos) == len(tiler.patches_lr) == 2
    src = replay_tile_noise(4242, 2, T, (1, 3, 64, 64))
    out = tiler.aggregation_sampling(noise_source=src, sampling_steps=5, eta=0.0).cpu()
    _, ah, _ = D.schedule("cosine", T)

    def tiles():
        res = []
        for k, (y0, x0) in enumerate(lr_origins):
            res.append(O.sample_superres(U.OracleUNet(seeded_sd), 1, img[0, :, y0:y0 + 32, x0:x0 + 32], T, ah, 2, 64, 5, 0.0,
                                         lambda i, shape, k=k: src(k, i, shape)).float())
        return torch.cat(res)
    want_tiles = _oracle("agg", tiles)
    want = A.aggregate(want_tiles, infos, A.gaussian_weight(64, 64), 64, 96)
    assert out.shape == want.shape == (1, 3, 64, 96)
    got_tiles = tiler.sample_tiles(noise_source=src, sampling_steps=5, eta=0.0).cpu()
    _check_chain("superres", "tiles S=5", impl, got_tiles, want_tiles)
    # the blend of the tiles: error relative to the tiles' amplitude (random weights drive the chains far outside [0, 1])
    err = ((out - want).abs().max() / want_tiles.abs().max()).item()
    print(f"ddim tiler [{impl}]: max abs error of the blended image / max |tile| {err:.3e}")
    assert err <= (3e-6 if impl == "mfma_f32" else 7e-5), err  # ~10x the measured 2.5e-7 / 6.9e-6


def test_ddim_eta0_chain_is_deterministic(dev, model):
    """Two eta = 0 chains from the same x_T give bit-identical images (no atomics in the forward or the update)."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    model.hip_engine().set_impl(IMPLS[-1])
    d = Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=200, device=dev, magnification_factor=2,
                  image_size=64, Degradation_type="DownBlur")
    lr1 = synthetic.tensor_uniform("ddim.det.lr", (3, 32, 32))
    xs = [d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(99), sampling_steps=20).cpu()
          for _ in range(2)]
    model.eval()
    assert torch.isfinite(xs[0]).all()
    assert torch.equal(xs[0], xs[1])
