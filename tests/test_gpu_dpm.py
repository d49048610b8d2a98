"""DPM-Solver++(2M) sampling on the GPU (drs_dpm_step, drs_blend_step_dpm and `Diffusion.sample(...,
sampling_steps=sampling_plan(S, "dpmpp_2m"))` of the three models, the tiler and the ensemble) against the float64 oracle of
tests/dpm_oracle.py, which drives the CPU oracle UNets from the same x_T."""
import math
import os

import pytest
import torch

import ddim_oracle as O
import dpm_oracle as P
import tile_chain_oracle as TC
from diffusionremotesensing_amd.sampling import sampling_plan
from conftest import longchain_state_dict, rel_errors, replay_noise_source
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U
from test_gpu_ddim import BOUNDS  # the DDIM chains' bounds per family, scaled below by the 2M move's gain

pytestmark = pytest.mark.gpu

IMPLS = [i for i in os.environ.get("DRS_TEST_IMPLS", "direct,mfma_f32,mfma_bf16x3").split(",") if i]
ULP = 2.0 ** -23
_ORACLE = {}


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


def _randn(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _r(ah, tq, t, tp):
    return (P.lam(ah, t) - P.lam(ah, tq)) / (P.lam(ah, tp) - P.lam(ah, t))


# (t_q | None, t, t_p): first-order moves without a history, second-order ones with r < 1 and r > 1, the moves to level 0
MOVES = ((None, 49, 42), (None, 1499, 1469), (60, 49, 30), (80, 49, 47), (1499, 1496, 1485), (1499, 1400, 1390), (11, 7, 1),
         (None, 1, 0), (None, 1499, 0))


def _step_scales(x, eps64, h, tq, t, tp, ah):
    cx, ce, cA, cB, cC = P.coefficients(tq, t, tp, ah)
    s_x = (cA * x.double()).abs() + (cB * eps64).abs() + (cC * h.double()).abs()
    s_0 = (cx * x.double()).abs() + (ce * eps64).abs()
    return s_x.max().item(), s_0.max().item()


# ---------------------------------------------------------------------------------------------
# the step kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_dpm_step_kernel_vs_float64_oracle(dev, kind):
    """drs_dpm_step against the float64 move: |x' - ref| / max(|A x| + |B eps| + |C x0_prev|) <= 1e-6 and |x0 - ref| /
    max(|cx x| + |ce eps|) <= 1e-6 - at most 8 fp32 roundings (3 coefficients, 3 products, 2 sums) of 2^-24 each, 4.8e-7 -
    bit-stable over calls.  A first-order move is handed a history of NaN: it must not read it."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule(kind, 1500)
    ah_d = ah.to(dev)
    rs = [_r(ah, tq, t, tp) for tq, t, tp in MOVES if tq is not None]
    assert min(rs) < 1 < max(rs), rs
    worst = [0.0, 0.0]
    for numel in (1920, 1, 3, 4, 5, 1027):  # two blocks of float4 groups; the tail alone; groups and tail
        x, ec, eu, h = (_randn(20 + k, (numel,)) for k in range(4))
        xd, ecd, eud, hd = (a.to(dev) for a in (x, ec, eu, h))
        for tq, t, tp in MOVES:
            for w in (None, 0.3, 3.0):
                eps64 = ec.double() if w is None else O.lerp64(eu, ec, w)
                want, want0 = P.step(x, eps64, h, tq, t, tp, ah)
                s_x, s_0 = _step_scales(x, eps64, h if tq is not None else torch.zeros_like(h), tq, t, tp, ah)
                outs = []
                for _ in range(2):
                    xs = xd.clone()
                    hs = hd.clone() if tq is not None else torch.full_like(hd, float("nan"))
                    hip_ops.dpm_step_(xs, ecd, hs, tq, t, tp, ah_d, eps_uncond=eud if w is not None else None,
                                      cfg_scale=w if w is not None else 0.0)
                    outs.append((xs.cpu(), hs.cpu()))
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (numel, tq, t, tp, w)
                err = (outs[0][0].double() - want).abs().max().item() / s_x
                err0 = (outs[0][1].double() - want0).abs().max().item() / s_0
                worst = [max(worst[0], err), max(worst[1], err0)]
                assert err <= 1e-6 and err0 <= 1e-6, (kind, numel, tq, t, tp, w, err, err0)
    print(f"dpm step kernel [{kind}]: worst normalised error x' {worst[0]:.3e}  x0 {worst[1]:.3e}")


def test_dpm_step_on_an_unaligned_view_and_through_reverse_step(dev):
    """Views that start 4 bytes into their buffers take the element-by-element path: the same bits as the aligned float4 one
    (one definition of the arithmetic, no contraction), and nothing is written outside the view.  `reverse_step_` dispatches
    on `hist`."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 1500)
    ah_d = ah.to(dev)
    n = 1027
    x, ec, eu, h = (_randn(40 + k, (n,)).to(dev) for k in range(4))
    for tq, t, tp in ((None, 49, 42), (60, 49, 30)):
        xa, ha = x.clone(), h.clone()
        hip_ops.dpm_step_(xa, ec, ha, tq, t, tp, ah_d, eps_uncond=eu, cfg_scale=3.0)
        bufs = [torch.full((n + 9,), 7.0, device=dev) for _ in range(4)]
        views = [b[1:n + 1] for b in bufs]
        assert all(v.data_ptr() % 16 == 4 for v in views)
        for v, src in zip(views, (x, ec, eu, h)):
            v.copy_(src)
        hip_ops.dpm_step_(views[0], views[1], views[3], tq, t, tp, ah_d, eps_uncond=views[2], cfg_scale=3.0)
        assert torch.equal(views[0], xa) and torch.equal(views[3], ha), (tq, t, tp)
        for b in bufs:
            assert (b[0] == 7.0).item() and (b[n + 1:] == 7.0).all().item()
        xr, hr = x.clone(), h.clone()
        hip_ops.reverse_step_(xr, ec, None, t, tp, alpha=None, alpha_hat=ah_d, beta=None, ddim=True, eps_uncond=eu, cfg_scale=3.0,
                              hist=hr, t_q=-1 if tq is None else tq)
        assert torch.equal(xr, xa) and torch.equal(hr, ha)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.dpm_step_(x, ec, h[:5], None, 49, 42, ah_d)
    with pytest.raises(RuntimeError, match="hist"):
        hip_ops.dpm_step_(x, ec, x, None, 49, 42, ah_d)
    buf = torch.zeros(n + 1, device=dev)
    for a, b in ((buf[:-1], buf[1:]), (buf[1:], buf[:-1])):  # shifted views of one buffer: refused before any launch
        with pytest.raises(RuntimeError, match="overlap"):
            hip_ops.dpm_step_(a, ec, b, None, 49, 42, ah_d)
    assert not buf.any().item()
    hip_ops.dpm_step_(buf[:8], ec[:8], buf[8:16], None, 49, 42, ah_d)  # neighbours in one buffer do not overlap
    with pytest.raises(RuntimeError, match="t_q"):
        hip_ops.dpm_step_(x, ec, h, 30, 49, 42, ah_d)


# ---------------------------------------------------------------------------------------------
# the driver on the device, without a network
# ---------------------------------------------------------------------------------------------
class _Schedule:
    def __init__(self, kind, T, dev):
        self.noise_steps, self.device = T, dev
        self.alpha, self.alpha_hat, self.beta = (a.to(dev) for a in D.schedule(kind, T))


class _Engine:
    def check_faults(self):
        pass


@pytest.mark.parametrize("kind,T", [("linear", 1000), ("cosine", 1500)])
def test_sample_chain_on_the_gaussian_problem(dev, kind, T):
    """`sample_chain` with the analytic eps of N(0, 0.25) data, shape (2, 3, 8, 8), S = 10: within 1e-5 (rel-L2) of the float64
    oracle chain given the same eps, and - as the oracle's - at most half the DDIM chain's error against the exact end point
    x_T sqrt(var_0 / var_L0) on the same logSNR levels."""
    from diffusionremotesensing_amd import sampling
    sch = _Schedule(kind, T, dev)
    _, ah, _ = D.schedule(kind, T)
    eps_fn = P.gauss_eps(ah)
    shape, S = (2, 3, 8, 8), 10
    calls = []

    def predict(engine, x, t_row, first):
        t = int(t_row[0])
        calls.append(t)
        return eps_fn(x, t)
    out = {}
    for solver in ("dpmpp_2m", "ddim"):
        out[solver] = sampling.sample_chain(sch, _Engine(), shape, predict, table_rows=2, noise_source=replay_noise_source(8),
                                            sampling_steps=sampling.sampling_plan(S, solver, "logsnr")).cpu()
    lv = P.logsnr_levels(ah, S)
    assert calls == lv + lv  # one model call per level, for either solver
    x_T = replay_noise_source(8)(T, shape)
    errs = {}
    for solver in ("dpmpp_2m", "ddim"):
        want = P.chain_on(eps_fn, x_T.double(), lv, ah, solver)
        _, e_l2 = rel_errors(out[solver], want)
        errs[solver] = rel_errors(out[solver], P.gauss_exact(x_T, ah, lv[0]))[1]
        print(f"gaussian chain [{kind} {solver}]: rel-L2 to the float64 chain {e_l2:.3e}, to the exact end point {errs[solver]:.3e}")
        assert e_l2 <= 1e-5, (kind, solver, e_l2)
    assert errs["dpmpp_2m"] <= 0.5 * errs["ddim"], errs


# ---------------------------------------------------------------------------------------------
# whole chains against the float64 oracle chain
# ---------------------------------------------------------------------------------------------
def _psnr_clamped(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).mean().item()
    return float("inf") if mse == 0 else -10 * math.log10(mse)


def _check_chain(family, what, impl, got, want, ah, S):
    """The DDIM bound of the family (tests/test_gpu_ddim.py: BOUNDS) times max_k (1 + 1 / r_k) of the chain's levels, in
    float64 from the schedule: the 2M move's gain on an error of eps relative to the DDIM move's, through k0 and C (about
    2.0 - 2.3 on such levels, 2.18 - 2.19 on these: DESIGN.md section 16; PSNR bound lowered by the same factor)."""
    g = P.max_gain(ah, P.logsnr_levels(ah, S))
    e_max, e_l2 = rel_errors(got, want)
    psnr = _psnr_clamped(got, want)
    if impl in ("direct", "mfma_f32"):
        l2_bound, psnr_bound = BOUNDS[family][0]
    elif impl == "mfma_bf16x3":
        l2_bound, psnr_bound = BOUNDS[family][1]
    else:  # opt-in mfma_f16
        l2_bound, psnr_bound = 5e-3, 40.0
    l2_bound, psnr_bound = l2_bound * g, psnr_bound - 20 * math.log10(g)
    print(f"dpm {what} [{impl}]: gain {g:.2f} max-rel {e_max:.3e} rel-L2 {e_l2:.3e} (bound {l2_bound:.2e}) PSNR {psnr:.1f} dB "
          f"(bound {psnr_bound:.1f})")
    assert torch.isfinite(got).all()
    assert e_l2 <= l2_bound and psnr >= psnr_bound, (what, impl, e_l2, l2_bound, psnr, psnr_bound)


def _superres(dev, sd, impl, T, image_size):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    return m, Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                        image_size=image_size, Degradation_type="DownBlur")


@pytest.mark.parametrize("impl", IMPLS)
def test_superres_dpm_chain_vs_oracle(dev, seeded_sd, impl):
    """n = 2, 64x64 (LR 32x32, x2), cosine T = 50, S = 10.  Measured on MI355X: see DESIGN.md section 16."""
    from diffusionremotesensing_amd import synthetic
    m, d = _superres(dev, seeded_sd, impl, 50, 64)
    lr1 = synthetic.tensor_uniform("dpm.sr.lr", (3, 32, 32))
    x = d.sample(2, m, lr1, input_channels=3, noise_source=replay_noise_source(606), sampling_steps=sampling_plan(10, "dpmpp_2m")).cpu()
    assert m.training  # same side effect as the other samplers
    _, ah, _ = D.schedule("cosine", 50)
    want = _oracle("sr", lambda: P.sample_superres(U.OracleUNet(seeded_sd), 2, lr1, 50, ah, 2, 64, 10, replay_noise_source(606)))
    _check_chain("superres", "superres T=50 S=10", impl, x, want, ah, 10)


@pytest.mark.parametrize("impl", IMPLS)
def test_superres_dpm_long_schedule_vs_oracle(dev, seeded_sd, impl):
    """configs[1]'s schedule (cosine T = 1500) in 20 steps at 32x32, n = 2, `output` damped as in the long DDIM chain test."""
    from diffusionremotesensing_amd import synthetic
    sd = longchain_state_dict(seeded_sd)
    m, d = _superres(dev, sd, impl, 1500, 32)
    lr1 = synthetic.tensor_uniform("dpm.long.lr", (3, 16, 16))
    x = d.sample(2, m, lr1, input_channels=3, noise_source=replay_noise_source(1501), sampling_steps=sampling_plan(20, "dpmpp_2m")).cpu()
    _, ah, _ = D.schedule("cosine", 1500)
    want = _oracle("long", lambda: P.sample_superres(U.OracleUNet(sd), 2, lr1, 1500, ah, 2, 32, 20, replay_noise_source(1501)))
    _check_chain("long", "superres T=1500 S=20", impl, x, want, ah, 20)


@pytest.mark.parametrize("impl", IMPLS)
def test_sar_dpm_chain_vs_oracle(dev, seeded_sd_sar, impl):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(seeded_sd_sar)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, image_size=64)
    sar1 = synthetic.tensor_uniform("dpm.sar", (2, 64, 64))
    x = d.sample(2, m, sar1, NDVI_channels=1, noise_source=replay_noise_source(304), sampling_steps=sampling_plan(10, "dpmpp_2m")).cpu()
    _, ah, _ = D.schedule("cosine", 50)
    want = _oracle("sar", lambda: P.sample_sar(U.OracleUNetSAR(seeded_sd_sar), 2, sar1, 50, ah, 64, 10, replay_noise_source(304)))
    _check_chain("sar", "sar T=50 S=10", impl, x, want, ah, 10)


@pytest.mark.parametrize("impl", IMPLS)
def test_generation_guided_dpm_chain_vs_oracle(dev, seeded_sd_gen, impl):
    """Classifier-free guidance 3: one 2n-row forward per step into the guided form of drs_dpm_step."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, image_size=32)
    cls = torch.tensor([2, 5])
    x = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(203), sampling_steps=sampling_plan(10, "dpmpp_2m")).cpu()
    _, ah, _ = D.schedule("cosine", 50)
    want = _oracle("gen", lambda: P.sample_generation(U.OracleUNetGeneration(seeded_sd_gen), 2, cls, 3, 50, ah, 32, 10,
                                                      replay_noise_source(203)))
    _check_chain("generation", "generation cfg=3 T=50 S=10", impl, x, want, ah, 10)


def test_default_spacing_and_ddim_on_logsnr_levels(dev, seeded_sd):
    """`spacing=None` is logsnr for the 2M solver; a DDIM plan with spacing="logsnr" is the DDIM kernel on those levels (against
    the float64 DDIM moves, the DDIM family's own bound); the 2M chain is deterministic to the bit."""
    from diffusionremotesensing_amd import synthetic
    m, d = _superres(dev, seeded_sd, "mfma_f32", 50, 64)
    lr1 = synthetic.tensor_uniform("dpm.sr.lr", (3, 32, 32))
    a, b = (d.sample(2, m, lr1, noise_source=replay_noise_source(606), sampling_steps=sampling_plan(10, "dpmpp_2m", sp)).cpu()
            for sp in (None, "logsnr"))
    assert torch.equal(a, b)
    u = d.sample(2, m, lr1, noise_source=replay_noise_source(606), sampling_steps=sampling_plan(10, "dpmpp_2m", "uniform")).cpu()
    assert torch.isfinite(u).all() and not torch.equal(a, u)
    x = d.sample(2, m, lr1, noise_source=replay_noise_source(606), sampling_steps=sampling_plan(10, spacing="logsnr")).cpu()
    _, ah, _ = D.schedule("cosine", 50)
    model = U.OracleUNet(seeded_sd)

    def eps_fn(xx, t):
        return model(xx, torch.full((2,), t, dtype=torch.long), lr1.unsqueeze(0), 2)
    want = P.chain(eps_fn, (2, 3, 64, 64), 50, ah, 10, replay_noise_source(606), solver="ddim")
    e_l2 = rel_errors(x, want)[1]
    print(f"ddim on logsnr levels: rel-L2 {e_l2:.3e}")
    assert e_l2 <= BOUNDS["superres"][0][0], e_l2


# ---------------------------------------------------------------------------------------------
# the per-step tiler
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_blend_step_dpm_kernel_vs_float64_oracle(dev, kind):
    """drs_blend_step_dpm against the float64 weighted mean + float64 move, at the bound of drs_dpm_step, bit-stable over
    calls: overlapping tiles, a partition, one tile, rows that are no multiple of 16 bytes (the element-by-element form)."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule(kind, 1500)
    ah_d = ah.to(dev)
    worst = 0.0
    for (h, w, ps, st, m, C) in ((24, 40, 16, 12, 2, 5), (16, 24, 8, 8, 2, 3), (8, 8, 8, 8, 2, 3), (16, 20, 8, 5, 1, 2),
                                 (20, 21, 8, 8, 1, 3)):
        infos, _ = A.tile_infos(h, w, ps, st, m)
        S, Hs, Ws = ps * m, h * m, w * m
        wt = A.gaussian_weight(S, S)
        x, hist = _randn(1, (C, Hs, Ws)), _randn(2, (C, Hs, Ws))
        eps_tiles = _randn(3, (len(infos), C, S, S))
        eps64 = TC.blend(eps_tiles, infos, wt, Hs, Ws)
        org = hip_ops.tile_origins([(i[0], i[2]) for i in infos], S, Hs, Ws, dev)
        xd, hd, ed, wd = x.to(dev), hist.to(dev), eps_tiles.to(dev), wt.to(dev)
        for tq, t, tp in MOVES:
            want, want0 = P.step(x, eps64, hist, tq, t, tp, ah)
            s_x, s_0 = _step_scales(x, eps64, hist if tq is not None else torch.zeros_like(hist), tq, t, tp, ah)
            outs = []
            for _ in range(2):
                unc = torch.zeros(1, dtype=torch.int32, device=dev)
                s = xd.clone()
                hs = hd.clone() if tq is not None else torch.full_like(hd, float("nan"))
                hip_ops.blend_step_(s, ed, org, wd, None, t, alpha_hat=ah_d, t_prev=tp, uncovered=unc, hist=hs, t_q=tq)
                assert int(unc.item()) == 0
                outs.append((s.cpu(), hs.cpu()))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (h, w, tq, t, tp)
            err = (outs[0][0].double() - want).abs().max().item() / s_x
            err0 = (outs[0][1].double() - want0).abs().max().item() / s_0
            worst = max(worst, err, err0)
            assert err <= 1e-6 and err0 <= 1e-6, (kind, (h, w, ps, st, m, C), tq, t, tp, err, err0)
    print(f"blend step dpm kernel [{kind}]: worst normalised error {worst:.3e}")
    with pytest.raises(RuntimeError, match="noise"):
        hip_ops.blend_step_(xd, ed, org, wd, xd, 10, alpha_hat=ah_d, t_prev=5, hist=hd)
    with pytest.raises(RuntimeError, match="hist"):
        hip_ops.blend_step_(xd, ed, org, wd, None, 10, alpha_hat=ah_d, t_prev=5, hist=hd[:1])


def test_one_tile_scene_agrees_with_diffusion_sample_on_the_2m_chain(dev, seeded_sd):
    """One tile covers the scene: its blended eps is (w e) / w, at most 1 ulp from the e `Diffusion.sample` uses, and the move's
    arithmetic is shared.  The bound of tests/test_gpu_tile_chain.py for such layouts, by the same reasoning: 8 ulp of max |x|
    per step."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    S = 5
    m, d = _superres(dev, seeded_sd, "mfma_f32", 8, 64)
    img = synthetic.tensor_uniform("dpm.tile.one", (1, 3, 32, 32)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 32, 2, d, dev)
    assert len(tiler.patches_lr) == 1
    got = tiler.sample_scene(noise_source=replay_noise_source(78), sampling_steps=sampling_plan(S, "dpmpp_2m")).cpu()
    assert m.training
    m.eval()
    want = d.sample(1, m, img[0], input_channels=3, noise_source=replay_noise_source(78), sampling_steps=sampling_plan(S, "dpmpp_2m")).cpu()
    assert got.shape == (3, 64, 64) and torch.isfinite(got).all()
    err = (got.double() - want[0].double()).abs().max().item()
    per_step = err / (ULP * want.abs().max().item()) / S
    print(f"one tile, 2M S={S}: max abs difference {err:.3e} = {per_step:.2f} ulp of max |x| per step")
    assert per_step <= 8, (err, per_step)


def test_joint_2m_chain_does_not_depend_on_the_tile_batch(dev, seeded_sd):
    """Six overlapping tiles (LR 48x56, patch 32, stride 16, x2), tile_batch 16 (one chunk) and 4 (two chunks, the last padded)
    agree to the bit on the exact-fp32 kernels; both `aggregation` modes take the solver."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    m, d = _superres(dev, seeded_sd, "mfma_f32", 50, 64)
    img = synthetic.tensor_uniform("dpm.tile.scene", (1, 3, 48, 56)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)
    assert len(tiler.patches_lr) == 6
    outs = {}
    for tile_batch in (16, 4):
        tiler.tile_batch = tile_batch
        outs[tile_batch] = tiler.sample_scene(noise_source=replay_noise_source(4060), sampling_steps=sampling_plan(6, "dpmpp_2m")).cpu()
        m.eval()
        assert outs[tile_batch].shape == (3, 96, 112) and torch.isfinite(outs[tile_batch]).all()
    assert torch.equal(outs[16], outs[4])
    ddim = tiler.sample_scene(noise_source=replay_noise_source(4060), sampling_steps=sampling_plan(6, spacing="logsnr")).cpu()
    assert not torch.equal(ddim, outs[4])
    per_step = tiler.aggregation_sampling(noise_source=replay_noise_source(4060), sampling_steps=sampling_plan(6, "dpmpp_2m"),
                                          aggregation="per_step").cpu()
    assert torch.equal(per_step[0], outs[4].clamp(0, 1))
    final = tiler.aggregation_sampling(noise_source=lambda tile, i, shape: _randn(900 + tile, shape),
                                       sampling_steps=sampling_plan(6, "dpmpp_2m")).cpu()
    assert final.shape == (1, 3, 96, 112) and torch.isfinite(final).all()


# ---------------------------------------------------------------------------------------------
# pass-through
# ---------------------------------------------------------------------------------------------
def test_sample_ensemble_passes_the_solver_through(dev, seeded_sd):
    """3 members of 2 LR images in chunks of 2 = `sample` calls on the same plan with 4 and 2 chains on the same noise source."""
    from diffusionremotesensing_amd import synthetic
    m, d = _superres(dev, seeded_sd, "mfma_f32", 20, 32)
    lr = synthetic.tensor_uniform("dpm.ensemble.lr", (2, 3, 16, 16)).to(dev)
    got = d.sample_ensemble(3, m, lr, input_channels=3, member_batch=2, sampling_steps=sampling_plan(5, "dpmpp_2m"),
                            noise_source=replay_noise_source(61))
    src = replay_noise_source(61)
    want = torch.cat([d.sample(2 * k, m, lr.repeat(k, 1, 1, 1), input_channels=3, noise_source=src, sampling_steps=sampling_plan(5, "dpmpp_2m")) for k in (2, 1)]).view(3, 2, 3, 32, 32)
    assert got.shape == (3, 2, 3, 32, 32) and torch.equal(got, want) and not torch.equal(got[0], got[1])
    ddim = d.sample_ensemble(3, m, lr, input_channels=3, member_batch=2, sampling_steps=5, noise_source=replay_noise_source(61))
    assert not torch.equal(got, ddim)
