"""Sampling with known pixels on the GPU: drs_inpaint_step and drs_renoise against the float64 oracle of
tests/inpaint_oracle.py and, bit for bit, against the update kernels they extend; `Diffusion.sample_known` of the three
models against the oracle chains, which drive the CPU oracle UNets with the same noise draws; `evaluate --known_fraction`."""
import json
import math
import os

import pytest
import torch

import ddim_oracle as O
import inpaint_oracle as I
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


def _oracle(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------
# the step kernel
# ---------------------------------------------------------------------------------------------
# (shape, bands of the mask): 480 elements per image in groups of four, and 63 elements - no group of four, one band
STEP_CASES = [((2, 3, 16, 20), 1), ((2, 3, 16, 20), 3), ((1, 1, 7, 9), 1)]
DDIM_MOVES = ((49, 42), (1499, 1469), (7, 1), (1, 0), (1499, 0))
ANCESTRAL_T = (1, 2, 750, 1499)


def _step_inputs(shape, cm, dev):
    g = torch.Generator().manual_seed(11 + shape[-1] + cm)
    x, ec, eu, z, known = (torch.randn(shape, generator=g) for _ in range(5))
    mask = (torch.rand((shape[0], cm) + shape[2:], generator=g) < 0.5).to(torch.uint8)
    assert 0 < int(mask.sum()) < mask.numel()
    return (x, ec, eu, z, known, mask), tuple(a.to(dev) for a in (x, ec, eu, z, known, mask))


def _check_move(host, devt, tables, tables_d, t, tp, eta, w, ancestral, worst):
    """One move on the mixed mask and on the all-zero mask against the oracle and the plain update kernel."""
    from diffusionremotesensing_amd import hip_ops
    x, ec, eu, z, known, mask = host
    xd, ecd, eud, zd, knd, md = devt
    alpha, ah, beta = tables
    al_d, ah_d, be_d = tables_d
    noise, noise_d = (z, zd) if tp > 0 else (None, None)
    eps64 = ec.double() if w is None else O.lerp64(eu, ec, w)
    cfg = {"eps_uncond": eud if w is not None else None, "cfg_scale": w if w is not None else 0.0}
    if ancestral:
        form = {"alpha": al_d, "beta": be_d}
        A, B, sigma = I.ancestral_coefficients(t, alpha, ah, beta)
        want = I.move(x, eps64, noise, known, mask, t, tp, ah, alpha=alpha, beta=beta)
        plain = xd.clone()
        if w is None:
            hip_ops.sampler_step_(plain, ecd, noise_d, t, al_d, ah_d, be_d)
        else:
            hip_ops.sampler_step_cfg_(plain, ecd, eud, w, noise_d, t, al_d, ah_d, be_d)
    else:
        form = {"t_prev": tp, "eta": eta}
        A, B, sigma = O.coefficients(t, tp, eta, ah)
        want = I.move(x, eps64, noise, known, mask, t, tp, ah, eta=eta)
        # (the plain kernel takes no noise at eta = 0: it would not read it)
        plain = hip_ops.ddim_step_(xd.clone(), ecd, noise_d if eta > 0 else None, t, tp, eta, ah_d, **cfg)
    outs = [hip_ops.inpaint_step_(xd.clone(), ecd, noise_d, knd, md, t, alpha_hat=ah_d, **form, **cfg) for _ in range(2)]
    tag = (t, tp, eta, w, ancestral)
    assert torch.equal(outs[0], outs[1]), tag
    m = mask.bool().expand_as(x)
    md_full = md.bool().expand_as(xd)
    # bit-equalities: the unknown elements are the plain kernel's, the known ones at level 0 are `known`
    assert torch.equal(outs[0][~md_full], plain[~md_full]), tag
    zero = hip_ops.inpaint_step_(xd.clone(), ecd, noise_d, knd, torch.zeros_like(md), t, alpha_hat=ah_d, **form, **cfg)
    assert torch.equal(zero, plain), tag
    if tp == 0:
        assert torch.equal(outs[0][md_full], knd[md_full]), tag
    # float64 oracle, each branch against its own scale
    got = outs[0].cpu().double()
    scale_u = (A * x.double()).abs() + (B * eps64).abs()
    if noise is not None and sigma > 0:
        scale_u = scale_u + (sigma * z.double()).abs()
    a, b = I.known_coefficients(tp, ah) if tp > 0 else (1.0, 0.0)
    scale_k = (a * known.double()).abs() + (b * z.double()).abs()
    err_u = ((got - want)[~m].abs().max() / scale_u.max()).item()
    err_k = ((got - want)[m].abs().max() / scale_k.max()).item()
    assert err_u <= 1e-6 and err_k <= 1e-6, (tag, err_u, err_k, A, B, sigma, a, b)
    worst[0], worst[1] = max(worst[0], err_u), max(worst[1], err_k)


@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("shape,cm", STEP_CASES)
def test_inpaint_step_kernel_vs_float64_oracle(dev, kind, shape, cm):
    """drs_inpaint_step, DDIM and ancestral form, with and without guidance: normalised error <= 1e-6 on each branch (unknown:
    / max(|A x| + |B eps| + |sigma z|), the bar of test_ddim_step_kernel_vs_float64_oracle; known: / max(|a known| + |b z|),
    three fp32 roundings = 1.8e-7), two calls bit-identical, the unknown elements (and the whole tensor under an all-zero
    mask) bit-identical to sampler_step_ / sampler_step_cfg_ / ddim_step_, the known elements at level 0 equal to `known`."""
    tables = D.schedule(kind, 1500)
    tables_d = tuple(a.to(dev) for a in tables)
    host, devt = _step_inputs(shape, cm, dev)
    worst = [0.0, 0.0]
    for w in (None, 0.3, 3.0):
        for t, tp in DDIM_MOVES:
            for eta in (0.0, 0.5, 1.0):
                _check_move(host, devt, tables, tables_d, t, tp, eta, w, False, worst)
        for t in ANCESTRAL_T:
            _check_move(host, devt, tables, tables_d, t, t - 1, 0.0, w, True, worst)
    print(f"inpaint step kernel [{kind} {shape} Cm={cm}]: worst normalised error unknown {worst[0]:.3e} known {worst[1]:.3e}")


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_renoise_kernel_vs_float64_oracle(dev, kind):
    """drs_renoise against the float64 jump: error / max(|A x| + |B z|) <= 1e-6, bit-stable, on a tensor with whole groups of
    four and on one of 63 elements (groups and a tail of three)."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule(kind, 1500)
    ah_d = ah.to(dev)
    worst = 0.0
    for shape in ((2, 3, 16, 20), (1, 1, 7, 9)):
        g = torch.Generator().manual_seed(13)
        x, z = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        xd, zd = x.to(dev), z.to(dev)
        for s, t in ((1, 2), (42, 49), (1469, 1499), (1, 1499)):
            A, B = I.renoise_coefficients(s, t, ah)
            want = I.renoise(x, z, s, t, ah)
            outs = [hip_ops.renoise_(xd.clone(), zd, s, t, ah_d).cpu() for _ in range(2)]
            assert torch.equal(outs[0], outs[1]), (s, t)
            scale = ((A * x.double()).abs() + (B * z.double()).abs()).max()
            err = ((outs[0].double() - want).abs().max() / scale).item()
            worst = max(worst, err)
            assert err <= 1e-6, (kind, shape, s, t, err, A, B)
    print(f"renoise kernel [{kind}]: worst normalised error {worst:.3e}")


def test_inpaint_ops_reject_bad_arguments(dev):
    from diffusionremotesensing_amd import hip_ops
    alpha, ah, beta = (a.to(dev) for a in D.schedule("cosine", 50))
    x = torch.zeros((2, 3, 8, 8), device=dev)
    e, z, kn = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    m1 = torch.zeros((2, 1, 8, 8), dtype=torch.uint8, device=dev)
    ddim = {"alpha_hat": ah, "t_prev": 5, "eta": 0.0}
    hip_ops.inpaint_step_(x, e, z, kn, m1, 10, **ddim)  # the good call
    for name, args in (("eps_cond", (torch.zeros((2, 3, 8, 7), device=dev), z, kn)),
                       ("noise", (e, torch.zeros((2, 3, 8, 7), device=dev), kn)),
                       ("known", (e, z, torch.zeros((1, 3, 8, 8), device=dev)))):
        with pytest.raises(RuntimeError, match=name + " has .* elements"):
            hip_ops.inpaint_step_(x, *args, m1, 10, **ddim)
    with pytest.raises(RuntimeError, match="mask"):
        hip_ops.inpaint_step_(x, e, z, kn, torch.zeros((2, 1, 8, 7), dtype=torch.uint8, device=dev), 10, **ddim)
    with pytest.raises(RuntimeError, match="mask of 2 bands"):
        hip_ops.inpaint_step_(x, e, z, kn, torch.zeros((2, 2, 8, 8), dtype=torch.uint8, device=dev), 10, **ddim)
    with pytest.raises(RuntimeError, match="uint8"):
        hip_ops.inpaint_step_(x, e, z, kn, m1.float(), 10, **ddim)
    # above level 0 the known pixels need z whatever eta is, in both forms
    with pytest.raises(RuntimeError, match="needs a noise tensor"):
        hip_ops.inpaint_step_(x, e, None, kn, m1, 10, **ddim)
    with pytest.raises(RuntimeError, match="needs a noise tensor"):
        hip_ops.inpaint_step_(x, e, None, kn, m1, 2, alpha_hat=ah, alpha=alpha, beta=beta)
    hip_ops.inpaint_step_(x, e, None, kn, m1, 10, alpha_hat=ah, t_prev=0, eta=1.0)
    hip_ops.inpaint_step_(x, e, None, kn, m1, 1, alpha_hat=ah, alpha=alpha, beta=beta)
    with pytest.raises(RuntimeError, match="t_prev < t"):
        hip_ops.inpaint_step_(x, e, z, kn, m1, 5, alpha_hat=ah, t_prev=5, eta=0.0)
    with pytest.raises(RuntimeError, match="outside"):
        hip_ops.inpaint_step_(x, e, z, kn, m1, 50, alpha_hat=ah, alpha=alpha, beta=beta)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.inpaint_step_(x, e, z, kn, m1, 10, alpha_hat=ah.cpu(), t_prev=5, eta=0.0)  # the tables live on the device
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.inpaint_step_(x, e, z, kn, m1, 10, alpha_hat=ah, alpha=alpha.cpu(), beta=beta)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.renoise_(x, z, 3, 9, ah.cpu())
    with pytest.raises(RuntimeError, match="noise has .* elements"):
        hip_ops.renoise_(x, torch.zeros((2, 3, 8, 7), device=dev), 3, 9, ah)
    for s, t in ((9, 9), (9, 3), (0, 3), (3, 50)):
        with pytest.raises(RuntimeError, match="s < t"):
            hip_ops.renoise_(x, z, s, t, ah)
    assert torch.equal(x.cpu(), torch.zeros(2, 3, 8, 8))  # no refused call wrote anything (the good ones map 0 to 0)


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
# rel-L2 and PSNR (dB, on the [0,1]-clamped images) bounds per chain: (exact fp32, split bf16) = 10x the rel-L2 and 20 dB
# under the PSNR measured on MI355X against the oracle, for the worse of direct / mfma_f32 and for mfma_bf16x3:
#   sar_ancestral  direct 1.19e-6 / 109.6 dB, mfma_f32 7.4e-7 / 111.2 dB, mfma_bf16x3 1.24e-5 / 91.9 dB
#   sar_resample   direct 8.8e-6 / 106.6 dB,  mfma_f32 1.89e-5 / 107.7 dB, mfma_bf16x3 6.1e-4 / 75.1 dB
#   superres       direct 6.9e-7 / 112.8 dB,  mfma_f32 6.7e-7 / 110.6 dB,  mfma_bf16x3 1.15e-5 / 89.3 dB
#   generation     direct 1.54e-6 / 111.3 dB, mfma_f32 1.77e-6 / 111.2 dB, mfma_bf16x3 2.57e-5 / 89.6 dB
# The fp32 bounds may not exceed the split-bf16 bounds of the same family in test_gpu_ddim.BOUNDS (sar 7e-5, superres 2.2e-4,
# generation 2e-4).  sar_resample is the one chain where 10x the measurement (1.9e-4) would: its fp32 bound is that cap, 7e-5
# (3.7x the measurement).  Its rel-L2 is ~25x that of the chain without resampling and of test_gpu_ddim's plain S = 10 chain
# (5.5e-7), while its PSNR is not lower and the kernels it adds are within 1.5e-7 of the oracle per move: the deviation sits in
# few pixels (max-rel 1.2e-4) that the seeded, untrained network amplifies over the three passes through every block.  That
# reading is a hypothesis; it has not been confirmed by an experiment.
BOUNDS = {"sar_ancestral": ((1.2e-5, 89.0), (1.3e-4, 71.0)), "sar_resample": ((7e-5, 86.0), (6.2e-3, 55.0)),
          "superres": ((6.9e-6, 90.0), (1.2e-4, 69.0)), "generation": ((1.8e-5, 91.0), (2.6e-4, 69.0))}


def _psnr_clamped(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).mean().item()
    return float("inf") if mse == 0 else -10 * math.log10(mse)


def _check_chain(case, impl, got, want, known, mask):
    e_max, e_l2 = rel_errors(got, want)
    psnr = _psnr_clamped(got, want)
    if impl in ("direct", "mfma_f32"):
        l2_bound, psnr_bound = BOUNDS[case][0]
    elif impl == "mfma_bf16x3":
        l2_bound, psnr_bound = BOUNDS[case][1]
    else:  # opt-in mfma_f16
        l2_bound, psnr_bound = 5e-3, 40.0
    print(f"inpaint {case} [{impl}]: max-rel {e_max:.3e} rel-L2 {e_l2:.3e} PSNR {psnr:.1f} dB")
    assert torch.isfinite(got).all()
    m = mask.bool().expand_as(got)
    assert torch.equal(got[m], known.expand_as(got)[m])  # the known pixels come back exactly
    assert not torch.equal(got[~m], known.expand_as(got)[~m])
    assert e_l2 <= l2_bound and psnr >= psnr_bound, (case, impl, e_l2, psnr)


def _cloud_mask(name, n, size):
    """Block masks hiding ~40 %: squares of an eighth of the side."""
    from diffusionremotesensing_amd import synthetic
    return synthetic.block_mask(name, n, size, 0.4, size // 8)


def _sar_model(dev, sd, impl):
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    return m


def _sar_case():
    from diffusionremotesensing_amd import synthetic
    return (synthetic.tensor_uniform("inpaint.sar", (2, 64, 64)), synthetic.tensor_uniform("inpaint.sar.known", (2, 1, 64, 64)),
            _cloud_mask("inpaint.sar.mask", 2, 64))


@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("case,S,eta,resample,jump", [("sar_ancestral", None, 0.0, 1, 1), ("sar_resample", 10, 0.5, 3, 2)])
def test_sar_inpaint_chain_vs_oracle(dev, seeded_sd_sar, impl, case, S, eta, resample, jump):
    """SAR -> NDVI, n = 2, 64 x 64, cosine T = 30: the ancestral chain without resampling (29 moves), and DDIM S = 10,
    eta = 0.5 with resample = 3, jump = 2 (26 moves down, 8 up)."""
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    m = _sar_model(dev, seeded_sd_sar, impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=30, device=dev, image_size=64)
    sar1, known, mask = _sar_case()
    x = d.sample_known(2, m, sar1, known, mask, NDVI_channels=1, noise_source=replay_noise_source(313), sampling_steps=S,
                       eta=eta, resample=resample, jump=jump).cpu()
    assert m.training  # same side effect as the plain sampler
    sched = D.schedule("cosine", 30)
    want = _oracle(case, lambda: I.sample_sar(U.OracleUNetSAR(seeded_sd_sar), 2, sar1, 30, sched, 64, S, eta,
                                              replay_noise_source(313), known, mask, resample, jump))
    _check_chain(case, impl, x, want, known, mask)


@pytest.mark.parametrize("impl", IMPLS)
def test_superres_inpaint_chain_vs_oracle(dev, seeded_sd, impl):
    """Super-resolution, n = 2, 64 x 64 (LR 32 x 32, x2), cosine T = 50, S = 7, eta = 0, resample = 2, jump = 3 (13 moves
    down, 2 up); one known image and one (S, S) bool mask broadcast over the chains and the bands."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, magnification_factor=2,
                  image_size=64, Degradation_type="DownBlur")
    lr1 = synthetic.tensor_uniform("inpaint.sr.lr", (3, 32, 32))
    known = synthetic.tensor_uniform("inpaint.sr.known", (3, 64, 64))
    mask = _cloud_mask("inpaint.sr.mask", 1, 64)[0, 0].bool()
    x = d.sample_known(2, m, lr1, known, mask, input_channels=3, noise_source=replay_noise_source(515), sampling_steps=7,
                       eta=0.0, resample=2, jump=3).cpu()
    sched = D.schedule("cosine", 50)
    want = _oracle("sr", lambda: I.sample_superres(U.OracleUNet(seeded_sd), 2, lr1, 50, sched, 2, 64, 7, 0.0,
                                                   replay_noise_source(515), known, mask, 2, 3))
    _check_chain("superres", impl, x, want, known.unsqueeze(0), mask)


@pytest.mark.parametrize("impl", IMPLS)
def test_generation_guided_inpaint_chain_vs_oracle(dev, seeded_sd_gen, impl):
    """Class-conditional inpainting with guidance 3: n = 2, 32 x 32, cosine T = 20, S = 6, eta = 1, resample = 2, jump = 2 (10
    moves down, 2 up), a mask per band and chain."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=20, device=dev, image_size=32)
    cls = torch.tensor([2, 5])
    known = synthetic.tensor_uniform("inpaint.gen.known", (2, 3, 32, 32))
    mask = _cloud_mask("inpaint.gen.mask", 6, 32).view(2, 3, 32, 32).float()
    x = d.sample_known(2, m, known, mask, target_class=cls, cfg_scale=3, input_channels=3,
                       noise_source=replay_noise_source(212), sampling_steps=6, eta=1.0, resample=2, jump=2).cpu()
    sched = D.schedule("cosine", 20)
    want = _oracle("gen", lambda: I.sample_generation(U.OracleUNetGeneration(seeded_sd_gen), 2, cls, 3, 20, sched, 32, 6, 1.0,
                                                      replay_noise_source(212), known, mask, 2, 2))
    _check_chain("generation", impl, x, want, known, mask)


def test_all_zero_mask_is_the_plain_sampler_bit_for_bit(dev, seeded_sd_sar):
    """SAR -> NDVI, ancestral, resample = 1, nothing known, same replay seed: the draws and the bits of the plain `sample`."""
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    m = _sar_model(dev, seeded_sd_sar, IMPLS[-1])
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=30, device=dev, image_size=64)
    sar1, known, mask = _sar_case()
    plain = d.sample(2, m, sar1, NDVI_channels=1, noise_source=replay_noise_source(77)).cpu()
    m.eval()
    zero = d.sample_known(2, m, sar1, known, torch.zeros_like(mask), NDVI_channels=1,
                          noise_source=replay_noise_source(77)).cpu()
    assert torch.isfinite(plain).all() and torch.equal(plain, zero)


def test_inpaint_chain_is_deterministic(dev, seeded_sd_sar):
    """Two identical chains with resampling give bit-identical images (no atomics in the forward, the move or the jump)."""
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    m = _sar_model(dev, seeded_sd_sar, IMPLS[-1])
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=30, device=dev, image_size=64)
    sar1, known, mask = _sar_case()
    xs = []
    for _ in range(2):
        m.eval()
        xs.append(d.sample_known(2, m, sar1, known, mask, NDVI_channels=1, noise_source=replay_noise_source(99),
                                 sampling_steps=8, eta=1.0, resample=2, jump=2).cpu())
    assert torch.isfinite(xs[0]).all() and torch.equal(xs[0], xs[1])


def test_evaluate_known_fraction(dev, seeded_sd_sar, tmp_path, monkeypatch, capsys):
    """`evaluate --task sar_to_ndvi --known_fraction 0.4` on two synthetic images: psnr_unknown is in the table and the JSON,
    finite, and not above the whole-image PSNR (the known pixels carry no error)."""
    from diffusionremotesensing_amd import evaluate
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "models_run" / "sar_known" / "weights")
    torch.save({"MODEL_STATE": seeded_sd_sar, "EPOCHS_RUN": 3}, tmp_path / "models_run" / "sar_known" / "weights" / "snapshot.pt")
    scores = evaluate.main(["--task", "sar_to_ndvi", "--model_name", "sar_known", "--image_size", "32", "--noise_steps", "10",
                            "--batch_size", "2", "--dataset_path", "synthetic:8", "--sampling_steps", "4", "--eta", "0.5",
                            "--known_fraction", "0.4", "--known_block", "4", "--resample", "2", "--jump", "2",
                            "--out", str(tmp_path / "k.json")])
    out = capsys.readouterr().out
    assert "PSNR unknown" in out and "40% of every image hidden" in out
    saved = json.load(open(tmp_path / "k.json"))
    assert saved["n"] == scores["n"] == 2 and set(saved["model"]) == {"psnr", "ssim", "psnr_unknown"}
    assert all(math.isfinite(v) for v in saved["model"].values()), saved["model"]
    assert len(saved["per_image"]["model"]["psnr_unknown"]) == 2
    for whole, hidden in zip(saved["per_image"]["model"]["psnr"], saved["per_image"]["model"]["psnr_unknown"]):
        assert math.isfinite(hidden) and whole >= hidden
    assert saved["model"]["psnr"] >= saved["model"]["psnr_unknown"]
    assert saved["args"]["known_fraction"] == 0.4
