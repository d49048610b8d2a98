"""v- and x0-prediction on the GPU: drs_noise_v_target and drs_pred_to_eps against the float64 oracle of
tests/prediction_oracle.py, `Diffusion(prediction=, x0_clip=)` chains of the three models and the tiler against the existing
float64 chains fed the converted eps, the analytic Gaussian problem in all three parameterisations, and the training step."""
import math
import os

import pytest
import torch

import dpm_oracle as P
import prediction_oracle as PO
import tile_chain_oracle as TC
from conftest import rel_errors, replay_noise_source
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U

pytestmark = pytest.mark.gpu

IMPL = "mfma_bf16x3"  # the arithmetic the shipped plans run; the conversion kernels are the same under every impl
KERNEL_BAR = 1e-6     # the project's bar for its step kernels (tests/test_gpu_ddim.py), error / largest sum of |terms|
SCHEDULES = {"cosine": 1500, "linear": 1000}
# one sweep of the capped grid is 2048 blocks x 256 threads x 4 elements: the last shape takes a second one, and a scalar tail
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 7), (2, 3, 16, 20), (2, 1, 1, 4097), (1, 1, 1, 2048 * 256 * 4 + 1029)]
CLIPS = (None, (0.0, 1.0), (-1.0, 1.0))
GUIDES = (None, 0.3, 3.0)
_ORACLE = {}  # float64 chains, computed once per case


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _levels(T):
    return [0, 1, 7, T // 2, T - 1]


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    # x0-like values around [0, 1] so that both clips bite on some elements and not on others
    return [torch.randn(shape, generator=g) for _ in range(3)] + [torch.rand(shape, generator=g) * 1.4 - 0.2]


def _norm_err(got, want, bound):
    top = bound.max().item()
    err = (got.double() - want).abs().max().item()
    return err / top if top > 0 else err


# ---------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_pred_to_eps_kernel_vs_float64_oracle(dev, kind, shape):
    """Every prediction x clip x guidance at t in {0, 1, 7, T/2, T-1}, mixed within the batch (the images' levels rotate through
    the list), normalised as test_ddim_step_kernel_vs_float64_oracle: error / max(sum of |terms|) <= 1e-6, the terms those of
    the clipped form with a clip.  The long image takes every case at T/2 and every level under one clip."""
    from diffusionremotesensing_amd import hip_ops
    T = SCHEDULES[kind]
    _, ah, _ = D.schedule(kind, T)
    ah_d = ah.to(dev)
    x, pc, pu, _ = _inputs(shape, 21)
    xd, pcd, pud = x.to(dev), pc.to(dev), pu.to(dev)
    n, lv, long = shape[0], _levels(T), shape[-1] > 100000
    rotations = [[lv[3]] * n] + [[lv[(i + r) % 5] for i in range(n)] for r in range(5)]
    worst = 0.0
    for r, levels in enumerate(rotations):
        t = torch.tensor(levels)
        td = t.to(dev)
        for pk in PO.KINDS:
            for clip in CLIPS:
                for w in GUIDES:
                    if long and r > 0 and (clip != (0.0, 1.0) or w is not None):
                        continue
                    if not long and r == 0:
                        continue
                    p64 = pc.double() if w is None else pu.double() + w * (pc.double() - pu.double())
                    want, bound = PO.to_eps(pk, p64, x, ah, t, clip)  # (the guided p as one term, as the DDIM step test has it)
                    guided = {"pred_uncond": pud, "cfg_scale": w} if w is not None else {}
                    out = torch.empty_like(pcd)
                    got = hip_ops.pred_to_eps_(pcd, xd, td, ah_d, pk, clip, out=out, **guided)
                    again = hip_ops.pred_to_eps_(pcd, xd, td, ah_d, pk, clip, out=torch.empty_like(pcd), **guided)
                    inplace = hip_ops.pred_to_eps_(pcd.clone(), xd, td, ah_d, pk, clip, **guided)
                    assert got is out and torch.equal(got, again) and torch.equal(got, inplace), (levels, pk, clip, w)
                    err = _norm_err(got.cpu(), want, bound)
                    worst = max(worst, err)
                    assert err <= KERNEL_BAR, (kind, shape, levels, pk, clip, w, err)
    print(f"pred_to_eps kernel [{kind} {shape}]: worst normalised error {worst:.3e}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_noise_v_target_kernel_vs_float64_oracle(dev, kind, shape):
    """x_t and v against the float64 oracle at the same levels, bit-stable over calls.  x_t carries the bits of
    `hip_ops.noise_images` wherever that kernel covers an image in one sweep of its own grid (chw <= 2048 * 256: every shape
    a trainer feeds it); beyond, its compiled loop fuses the sum of its earlier sweeps into a multiply-add and leaves its last
    one unfused, so there x_t is held to the documented formula fl(a x0) + fl(b eps) instead - as at every other shape -
    stated with torch's fp32 operators."""
    from diffusionremotesensing_amd import hip_ops
    T = SCHEDULES[kind]
    _, ah, _ = D.schedule(kind, T)
    ah_d = ah.to(dev)
    _, eps, _, x0 = _inputs(shape, 22)
    x0d, epsd = x0.to(dev), eps.to(dev)
    n, lv, long = shape[0], _levels(T), shape[-1] > 100000
    worst = 0.0
    for r in range(5):
        if long and r not in (0, 3):
            continue
        t = torch.tensor([lv[(i + r) % 5] for i in range(n)])
        td = t.to(dev)
        x_t, v = hip_ops.noise_v_target(x0d, epsd, td, ah_d)
        x_t2, v2 = hip_ops.noise_v_target(x0d, epsd, td, ah_d)
        assert torch.equal(x_t, x_t2) and torch.equal(v, v2)
        a = torch.sqrt(ah_d[td]).view(-1, 1, 1, 1)
        b = torch.sqrt(1.0 - ah_d[td]).view(-1, 1, 1, 1)
        assert torch.equal(x_t, a * x0d + b * epsd) and torch.equal(v, a * epsd - b * x0d), (kind, shape, t.tolist())
        if x0[0].numel() <= 2048 * 256:
            assert torch.equal(x_t, hip_ops.noise_images(x0d, epsd, td, ah_d)), (kind, shape, t.tolist())
        want_x, want_v, bound_x, bound_v = PO.v_target(x0, eps, ah, t)
        ex, ev = _norm_err(x_t.cpu(), want_x, bound_x), _norm_err(v.cpu(), want_v, bound_v)
        worst = max(worst, ex, ev)
        assert ex <= KERNEL_BAR and ev <= KERNEL_BAR, (kind, shape, t.tolist(), ex, ev)
    print(f"noise_v_target kernel [{kind} {shape}]: worst normalised error {worst:.3e}")


def test_x_t_is_noise_images_at_a_training_shape(dev):
    """The batch of the training tests and the benchmark's image: `noise_v_target`'s x_t is `noise_images`', bit for bit."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 1500)
    for shape in ((2, 3, 32, 32), (3, 3, 256, 256)):
        _, eps, _, x0 = _inputs(shape, 23)
        t = torch.tensor([1, 700, 1499][:shape[0]]).to(dev)
        x_t, _ = hip_ops.noise_v_target(x0.to(dev), eps.to(dev), t, ah.to(dev))
        assert torch.equal(x_t, hip_ops.noise_images(x0.to(dev), eps.to(dev), t, ah.to(dev)))


@pytest.mark.parametrize("pk", PO.KINDS)
def test_planted_values(dev, pk):
    """NaN and +-inf in the prediction come out non-finite - never clamped into range - and leave their neighbours alone;
    a prediction exactly at lo or hi is inside the range; one past it gives the bits of the bound itself."""
    from diffusionremotesensing_amd import hip_ops
    T = 1500
    _, ah, _ = D.schedule("cosine", T)
    ah_d = ah.to(dev)
    x, p, _, _ = _inputs((2, 1, 5, 7), 24)
    t = torch.tensor([7, T // 2]).to(dev)
    bad = p.clone()
    spots = [(0, 0, 0, 0), (0, 0, 2, 3), (1, 0, 4, 6), (1, 0, 1, 1)]
    for spot, val in zip(spots, (math.nan, math.inf, -math.inf, math.nan)):
        bad[spot] = val
    mask = torch.zeros_like(p, dtype=torch.bool)
    for spot in spots:
        mask[spot] = True
    for clip in CLIPS:
        clean = hip_ops.pred_to_eps_(p.to(dev), x.to(dev), t, ah_d, pk, clip).cpu()
        got = hip_ops.pred_to_eps_(bad.to(dev), x.to(dev), t, ah_d, pk, clip).cpu()
        assert not torch.isfinite(got[mask]).any(), (pk, clip, got[mask])
        assert torch.equal(got[~mask], clean[~mask]) and torch.isfinite(clean).all()
        for uw in (0.3, 3.0):  # a non-finite unconditional prediction reaches the output as well
            g2 = hip_ops.pred_to_eps_(p.to(dev), x.to(dev), t, ah_d, pk, clip, pred_uncond=bad.to(dev), cfg_scale=uw).cpu()
            assert not torch.isfinite(g2[mask]).any() and torch.isfinite(g2[~mask]).all()
    if pk == "x0":
        lo, hi = 0.0, 1.0
        edge = p.clone()
        edge[0, 0, 0, :4] = torch.tensor([lo, hi, lo - 1.0, hi + 1.0])
        at = edge.clone()
        at[0, 0, 0, :4] = torch.tensor([lo, hi, lo, hi])
        inside = (at >= lo) & (at <= hi)
        clipped = hip_ops.pred_to_eps_(edge.to(dev), x.to(dev), t, ah_d, pk, (lo, hi)).cpu()
        free = hip_ops.pred_to_eps_(at.to(dev), x.to(dev), t, ah_d, pk, None).cpu()
        assert inside[0, 0, 0, :4].all() and torch.equal(clipped[inside], free[inside])


def test_levels_outside_the_table_give_nan_images(dev):
    from diffusionremotesensing_amd import hip_ops
    T = 1000
    _, ah, _ = D.schedule("linear", T)
    ah_d = ah.to(dev)
    for shape in ((3, 1, 5, 7), (3, 3, 16, 20)):
        x, p, u, x0 = (a.to(dev) for a in _inputs(shape, 25))
        good, bad = torch.tensor([5, 5, 5]).to(dev), torch.tensor([-1, 5, T]).to(dev)
        for pk in PO.KINDS:
            for clip in (None, (0.0, 1.0)):
                for guided in ({}, {"pred_uncond": u, "cfg_scale": 3.0}):
                    want = hip_ops.pred_to_eps_(p.clone(), x, good, ah_d, pk, clip, **guided)
                    got = hip_ops.pred_to_eps_(p.clone(), x, bad, ah_d, pk, clip, **guided)
                    assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all() and torch.equal(got[1], want[1])
        wx, wv = hip_ops.noise_v_target(x0, p, good, ah_d)
        gx, gv = hip_ops.noise_v_target(x0, p, bad, ah_d)
        for got, want in ((gx, wx), (gv, wv)):
            assert torch.isnan(got[0]).all() and torch.isnan(got[2]).all() and torch.equal(got[1], want[1])
    torch.cuda.synchronize()


def test_wrappers_reject_bad_tensors(dev):
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 50)
    ah_d = ah.to(dev)
    x = torch.zeros((2, 3, 8, 8), device=dev)
    t = torch.ones(2, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(x.clone(), torch.zeros((2, 3, 8, 7), device=dev), t, ah_d, "v")
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(x.clone(), x, t, ah_d, "v", pred_uncond=torch.zeros((2, 3, 8, 7), device=dev), cfg_scale=1.0)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(x.clone(), x, torch.ones(3, dtype=torch.int64, device=dev), ah_d, "v")
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.pred_to_eps_(x.clone(), x, t, ah, "v")  # the table must live on the device
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.pred_to_eps_(torch.zeros((2, 3, 8, 16), device=dev)[..., ::2], x, t, ah_d, "v")  # the state is used as it is
    with pytest.raises(RuntimeError, match="int64"):
        hip_ops.pred_to_eps_(x.clone(), x, t.int(), ah_d, "v")
    with pytest.raises(ValueError, match="lo < hi"):
        hip_ops.pred_to_eps_(x.clone(), x, t, ah_d, "v", (1.0, 1.0))
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.noise_v_target(x, torch.zeros((2, 3, 8, 7), device=dev), t, ah_d)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.noise_v_target(x, x, torch.ones(3, dtype=torch.int64, device=dev), ah_d)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.noise_v_target(x, x, t, ah)
    # a view that starts elsewhere in its 16-byte line than the state: element by element, the same values
    buf = torch.randn(2 * 3 * 8 * 8 + 1, device=dev)
    p, shifted = buf[:-1].view(2, 3, 8, 8).clone(), buf[1:].view(2, 3, 8, 8)
    shifted.copy_(p)
    assert torch.equal(hip_ops.pred_to_eps_(shifted, x + 0.5, t, ah_d, "x0", (0.0, 1.0)),
                       hip_ops.pred_to_eps_(p, x + 0.5, t, ah_d, "x0", (0.0, 1.0)))


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
# rel-L2 and PSNR (dB, on the [0, 1]-clamped images) of the chains against the float64 oracle chains, per family: (bound on
# rel-L2, bound on PSNR) = 10x the rel-L2 and 20 dB under the PSNR measured on MI355X for the family's worst case, the margin of
# BOUNDS in tests/test_gpu_ddim.py and for its reason (box-to-box and summation-order variation).  Measured (rel-L2 / PSNR):
#   superres (16 chains)   v: 4.9e-6 .. 6.3e-6 / 108.7 .. 111.3 dB;  x0: 1.8e-5 .. 2.0e-5 / 103.4 .. 103.7 dB
#                          worst: x0, ancestral, clip (0, 1): 1.98e-5 / 103.4 dB
#   sar v DDIM 7, clip (-1, 1)            3.2e-6 / 111.8 dB      generation v, cfg 3, DDIM 7      9.0e-6 / 101.4 dB
#   sample_known v DDIM 7, clip (0, 1)    4.3e-6 / 112.6 dB      tiler v DDIM 7, clip (0, 1)      per_step 5.8e-6 / 110.5 dB,
#   Gaussian problem, DDIM 10             eps 4.1e-7 / 139.0 dB, v 5.1e-7 / 137.2 dB, x0 6.7e-7 / 134.7 dB    final 5.7e-6 / 110.6 dB
BOUNDS = {"superres": (2.0e-4, 83.0), "sar": (3.2e-5, 91.0), "generation": (9.0e-5, 81.0), "known": (4.4e-5, 92.0),
          "tiler": (5.8e-5, 90.0), "gauss": (6.7e-6, 114.0)}
SAMPLERS = {"ancestral": ("ancestral",), "ddim7_eta0": ("ddim", 7, 0.0), "ddim7_eta1": ("ddim", 7, 1.0), "dpmpp10": ("dpmpp_2m", 10)}


def _psnr_clamped(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).mean().item()
    return float("inf") if mse == 0 else -10 * math.log10(mse)


def _check_chain(family, what, got, want):
    e_max, e_l2 = rel_errors(got, want)
    psnr = _psnr_clamped(got, want)
    print(f"prediction chain {what}: max-rel {e_max:.3e} rel-L2 {e_l2:.3e} PSNR {psnr:.1f} dB (max |x| {want.abs().max():.3g})")
    assert torch.isfinite(got).all()
    assert e_l2 <= BOUNDS[family][0] and psnr >= BOUNDS[family][1], (what, e_l2, psnr)


def _sampling_args(sampler):
    from diffusionremotesensing_amd.sampling import sampling_plan
    if sampler[0] == "ancestral":
        return {}
    if sampler[0] == "ddim":
        return {"sampling_steps": sampler[1], "eta": sampler[2]}
    return {"sampling_steps": sampling_plan(sampler[1], solver="dpmpp_2m")}


def _oracle(key, fn):
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


@pytest.fixture(scope="module")
def model(dev, seeded_sd):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    return m


def _superres(model, dev, T=50, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                     image_size=64, Degradation_type="DownBlur", **kw)


@pytest.mark.parametrize("clip", [None, (0.0, 1.0)], ids=["noclip", "clip01"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("pk", ["v", "x0"])
def test_superres_chain_vs_oracle(dev, model, seeded_sd, pk, sampler, clip):
    """n = 2, 64x64 (LR 32x32, x2), cosine T = 50, the seeded weights read as a v / x0 network; eta = 0 chains twice, bit for
    bit."""
    from diffusionremotesensing_amd import synthetic
    d = _superres(model, dev, prediction=pk, x0_clip=clip)
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    args = _sampling_args(SAMPLERS[sampler])
    x = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
    model.eval()
    if sampler in ("ddim7_eta0", "dpmpp10"):
        again = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
        model.eval()
        assert torch.equal(x, again)
    sched = D.schedule("cosine", 50)
    want = _oracle(("sr", pk, sampler, clip), lambda: PO.chain(
        pk, clip, PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2), (2, 3, 64, 64), 50, sched, SAMPLERS[sampler],
        replay_noise_source(505)))
    _check_chain("superres", f"superres {pk} {sampler} clip={clip}", x, want)


def test_default_chain_is_unchanged_by_the_new_arguments(dev, model):
    """prediction="eps" with no clip launches nothing new: the bits of a `Diffusion` built without the arguments; and an eps
    network under a clip that cannot bite gives the converted chain (x -> x0 -> eps: the same chain up to rounding)."""
    from diffusionremotesensing_amd import synthetic
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    outs = []
    for kw in ({}, {"prediction": "eps", "x0_clip": None}, {"x0_clip": (-1e30, 1e30)}):
        d = _superres(model, dev, **kw)
        outs.append(d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(7), sampling_steps=7).cpu())
        model.eval()
    assert torch.equal(outs[0], outs[1])
    assert rel_errors(outs[2], outs[0])[1] < 1e-3 and not torch.equal(outs[2], outs[0])


def test_sar_v_chain_vs_oracle(dev, seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(seeded_sd_sar)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, image_size=64, prediction="v",
                  x0_clip=(-1.0, 1.0))
    sar1 = synthetic.tensor_uniform("ddim.sar", (2, 64, 64))
    x = d.sample(2, m, sar1, NDVI_channels=1, noise_source=replay_noise_source(303), sampling_steps=7, eta=0.0).cpu()
    want = PO.chain("v", (-1.0, 1.0), PO.sar_pred_fn(U.OracleUNetSAR(seeded_sd_sar), 2, sar1), (2, 1, 64, 64), 50,
                    D.schedule("cosine", 50), ("ddim", 7, 0.0), replay_noise_source(303))
    _check_chain("sar", "sar v ddim7 clip=(-1, 1)", x, want)


def test_generation_guided_v_chain_vs_oracle(dev, seeded_sd_gen):
    """cfg_scale = 3: the conversion launch forms the guided v from both halves of the 2n-row forward (the t row is 2n wide)
    and the update gets one eps."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, image_size=64, prediction="v")
    cls = torch.tensor([2, 5])
    x = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(202),
                 sampling_steps=7, eta=0.0).cpu()
    want = PO.chain("v", None, PO.generation_pred_fn(U.OracleUNetGeneration(seeded_sd_gen), 2, cls, 3), (2, 3, 64, 64), 50,
                    D.schedule("cosine", 50), ("ddim", 7, 0.0), replay_noise_source(202))
    _check_chain("generation", "generation v cfg=3 ddim7", x, want)


def test_sample_known_v_chain_vs_oracle(dev, model, seeded_sd):
    """Known pixels on a v chain (DDIM S = 7, eta = 0) against tests/inpaint_oracle.py fed the converted eps."""
    import inpaint_oracle as I
    from diffusionremotesensing_amd import synthetic
    d = _superres(model, dev, prediction="v", x0_clip=(0.0, 1.0))
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    known = synthetic.tensor_uniform("prediction.known", (3, 64, 64))
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :24] = True
    x = d.sample_known(2, model, lr1, known, mask, input_channels=3, noise_source=replay_noise_source(606),
                       sampling_steps=7, eta=0.0).cpu()
    model.eval()
    sched = D.schedule("cosine", 50)
    eps_fn = PO.eps_fn_of("v", (0.0, 1.0), sched[1], PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2))
    want = I.chain(eps_fn, (2, 3, 64, 64), 50, *sched, 7, 0.0, replay_noise_source(606), known, mask)
    assert torch.equal(x[:, :, :, :24], known[None, :, :, :24].expand(2, -1, -1, -1))
    _check_chain("known", "sample_known v ddim7 clip=(0, 1)", x, want)


@pytest.mark.parametrize("mode", ["per_step", "final"])
def test_tiler_v_scene_vs_oracle(dev, model, seeded_sd, mode):
    """A scene of 2 x 2 tiles (LR 48x48, patch 32, stride 16, x2) on a v network with the clip (0, 1): the joint chain converts
    each chunk against the tiles it gathered (two chunks: tile_batch = 2); the final mode's tile chains convert in the chain."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T, S, clip = 50, 7, (0.0, 1.0)
    d = _superres(model, dev, T, prediction="v", x0_clip=clip)
    img = synthetic.tensor_uniform("prediction.scene", (1, 3, 48, 48))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(48, 48, 32, 16, 2)
    assert [tuple(i) for i in tiler.patches_sr_infos] == infos and len(infos) == 4
    lr_tiles = torch.stack([img[0, :, y0:y0 + 32, x0:x0 + 32] for (y0, x0) in lr_origins])
    sched = D.schedule("cosine", T)
    net = U.OracleUNet(seeded_sd)
    if mode == "per_step":
        tiler.tile_batch = 2
        got = tiler.sample_scene(noise_source=replay_noise_source(707), sampling_steps=S, eta=0.0).cpu()

        def eps_fn(x_tiles, t, rng):
            pred = net(x_tiles, torch.full((rng[1] - rng[0],), t, dtype=torch.long), lr_tiles[rng[0]:rng[1]], 2)
            return PO.to_eps("v", pred, x_tiles, sched[1], t, clip)[0]
        want = TC.chain(eps_fn, 3, 96, 96, infos, A.gaussian_weight(64, 64), T, sched, replay_noise_source(707), S, 0.0)
    else:
        from conftest import replay_tile_noise
        src = replay_tile_noise(808, 4, T, (1, 3, 64, 64))
        got = tiler.sample_tiles(noise_source=src, sampling_steps=S, eta=0.0).cpu()
        want = torch.cat([PO.chain("v", clip, PO.superres_pred_fn(net, 1, lr_tiles[k], 2), (1, 3, 64, 64), T, sched,
                                   ("ddim", S, 0.0), lambda i, shape, k=k: src(k, i, shape)) for k in range(4)])
    model.eval()
    _check_chain("tiler", f"tiler {mode} v ddim7 clip=(0, 1)", got, want)


# ---------------------------------------------------------------------------------------------
# consistency without a network
# ---------------------------------------------------------------------------------------------
class _StubEngine:
    def check_faults(self):
        pass


@pytest.mark.parametrize("pk", PO.KINDS)
def test_gaussian_problem_in_every_parameterisation(dev, pk):
    """`sample_chain` with no network: the optimal predictor of per-pixel N(0, VAR0) data, stated as eps, v and x0, over DDIM
    S = 10 from one x_T.  Each chain against the float64 chain on the same predictor; the three also end at the same image -
    the probability-flow ODE's - up to the rounding of their different routes."""
    import types

    import ddim_oracle as O
    from diffusionremotesensing_amd import sampling
    T, S, shape = 50, 10, (2, 3, 16, 20)
    alpha, ah, beta = D.schedule("cosine", T)
    pred = PO.gauss_pred(pk, ah)
    sched = types.SimpleNamespace(noise_steps=T, alpha=alpha.to(dev), alpha_hat=ah.to(dev), beta=beta.to(dev), device=dev,
                                  prediction=pk, x0_clip=None)

    def predict(engine, x, t, first):
        level = int(t[0].item())
        return pred(x.cpu(), level).to(dev).contiguous()
    got = sampling.sample_chain(sched, _StubEngine(), shape, predict, table_rows=shape[0], noise_source=replay_noise_source(11),
                                sampling_steps=S, eta=0.0).cpu()
    want = O.chain(PO.eps_fn_of(pk, None, ah, pred), shape, T, ah, S, 0.0, replay_noise_source(11))
    _check_chain("gauss", f"gaussian {pk} ddim10", got, want)
    plain = _oracle("gauss", lambda: O.chain(P.gauss_eps(ah), shape, T, ah, S, 0.0, replay_noise_source(11)))
    assert rel_errors(want, plain)[1] <= 1e-6  # one problem, three statements (the fp32 predictor's rounding apart)


# ---------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------
GRAD_REL = 2.0 ** -22  # tests/test_gpu_loss.py: the coefficient w_b c / (B n) is rounded once, its product with d once


@pytest.mark.parametrize("weighting", ["none", "min_snr"])
@pytest.mark.parametrize("pk", ["v", "x0"])
def test_train_step_target_and_gradient(dev, seeded_sd, tmp_path, pk, weighting):
    """One epoch (one training batch of 2 x 3 x 32 x 32, one validation batch) with the fused loss.  The target both loops
    hand the loss is the one `_noised_target` made, and it is the oracle's: at the kernels' bar for v (error / largest sum of
    |terms| <= 1e-6), the clean batch itself for x0.  The gradient handed to the UNet backward is the float64 autograd
    gradient of the weighted MSE against that target within 2^-22 per element.  (Per element and relative, the bar has a
    meaning only against the fp32 target the loss read: d = pred - target cancels, so a target one ulp away moves d by
    ulp / |d|, which no arithmetic bounds.  The target is therefore held to the oracle by its own bar, and the gradient to
    the target.)"""
    from torch.utils.data import DataLoader
    from diffusionremotesensing_amd import hip_ops
    from diffusionremotesensing_amd.losses import DiffusionLoss
    from diffusionremotesensing_amd.superres_feeds import SyntheticSuperresDataset
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    d = Diffusion("cosine", m.to(dev), str(tmp_path / "snapshot.pt"), noise_steps=50, device=dev, magnification_factor=2,
                  image_size=32, Degradation_type="DownBlur", prediction=pk)
    made, launched, seen = [], [], {}
    noised_target, predict, launch, nvt = d._noised_target, d._predict, DiffusionLoss._launch, hip_ops.noise_v_target

    def noised_target_seen(x0, t):
        x_t, target = noised_target(x0, t)
        made.append({"x0": x0, "t": t, "x_t": x_t, "target": target})
        return x_t, target

    def predict_seen(net, x_t, t, cond):
        out = predict(net, x_t, t, cond)
        if out.requires_grad:
            seen["pred"] = out.detach().clone()
            out.register_hook(lambda g: seen.__setitem__("grad", g.detach().clone()))
        return out

    def launch_seen(self, pred, target, t, sample_w, with_grad):
        launched.append((target, with_grad))
        return launch(self, pred, target, t, sample_w, with_grad)

    def nvt_seen(x0, eps, t, alpha_hat):
        seen.setdefault("eps", []).append(eps)
        return nvt(x0, eps, t, alpha_hat)
    d._noised_target, d._predict = noised_target_seen, predict_seen
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(DiffusionLoss, "_launch", launch_seen)
        mp.setattr(hip_ops, "noise_v_target", nvt_seen)
        kw = {"loss_weighting": "min_snr", "min_snr_gamma": 5.0} if weighting == "min_snr" else {"loss_bins": 4}
        d.train(lr=1e-4, epochs=1, check_preds_epoch=1, train_loader=DataLoader(SyntheticSuperresDataset(2, 3, 32, 2, seed=5), 2),
                val_loader=DataLoader(SyntheticSuperresDataset(2, 3, 32, 2, seed=6), 2), patience=10, loss="MSE", verbose=False,
                **kw)
    # training and validation: the same helper, and its target is what the loss read
    assert len(made) == 2 and [w for _, w in launched] == [True, False]
    assert all(tg is mk["target"] for (tg, _), mk in zip(launched, made))
    for k, mk in enumerate(made):
        if pk == "x0":
            assert mk["target"] is mk["x0"]
        else:
            eps = seen["eps"][k]
            want_x, want_v, bound_x, bound_v = PO.v_target(mk["x0"].cpu(), eps.cpu(), d.alpha_hat.cpu(), mk["t"].cpu())
            assert _norm_err(mk["target"].cpu(), want_v, bound_v) <= KERNEL_BAR
            assert _norm_err(mk["x_t"].cpu(), want_x, bound_x) <= KERNEL_BAR
            assert torch.equal(mk["x_t"], hip_ops.noise_images(mk["x0"], eps, mk["t"], d.alpha_hat))
    # the gradient of the training step
    tgt, t = made[0]["target"].double(), made[0]["t"]
    w = PO.weights(pk, d.alpha_hat.cpu(), 5.0).float().double().to(dev)[t] if weighting == "min_snr" else torch.ones(2, device=dev).double()
    p = seen["pred"].double().requires_grad_()
    (w * ((p - tgt) ** 2).flatten(1).mean(1)).mean().backward()
    got, want = seen["grad"].double().cpu(), p.grad.cpu()
    zero = want == 0
    err = ((got - want).abs() / want.abs().clamp_min(1e-300))[~zero]
    print(f"train_step {pk} {weighting}: worst relative gradient error {err.max().item():.3e} (bar {GRAD_REL:.3e})")
    assert (got[zero] == 0).all() and err.max().item() <= GRAD_REL


_RUN = ["--image_size", "32", "--noise_steps", "10", "--epochs", "1", "--batch_size", "2", "--check_preds_epoch", "1", "--loss", "MSE",
        "--dataset_path", "synthetic:4", "--prediction", "v", "--loss_weighting", "min_snr", "--loss_bins", "4",
        "--save_train_state", "--sampling_steps", "3"]


@pytest.mark.parametrize("trainer", ["superres", "sar", "generation"])
def test_trainer_command_line_with_v_prediction(dev, tmp_path, monkeypatch, capsys, trainer):
    """One epoch of the trainer's command line as a v network: it runs, writes PREDICTION, resumes, and refuses to resume as
    an eps network."""
    import importlib
    mod = importlib.import_module("diffusionremotesensing_amd." + {
        "superres": "train_diffusion_superres", "sar": "train_diffusion_SAR_TO_NDVI",
        "generation": "generate_new_imgs.train_diffusion_generation"}[trainer])
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    name = "v_" + trainer
    argv = _RUN + ["--model_name", name] + (["--magnification_factor", "2"] if trainer == "superres" else [])
    mod.main(argv)
    weights = tmp_path / "models_run" / name / "weights"
    snap = torch.load(weights / "snapshot.pt")
    assert set(snap) == {"MODEL_STATE", "EPOCHS_RUN", "PREDICTION"} and snap["PREDICTION"] == "v"
    assert os.path.exists(weights / "train_state.pt")
    out = capsys.readouterr().out
    assert "loss by timestep bin" in out
    mod.main([a if a != "1" or argv[i - 1] != "--epochs" else "2" for i, a in enumerate(argv)])  # one more epoch
    out = capsys.readouterr().out
    assert "Resuming the training state" in out and "Epoch 1: Running Train" in out and "Epoch 0: Running Train" not in out
    as_eps = [a for i, a in enumerate(argv) if a not in ("--prediction",) and argv[i - 1] != "--prediction"]
    with pytest.raises(ValueError, match="predicts 'v'"):
        mod.main(as_eps)
