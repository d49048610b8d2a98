"""Zero-terminal-SNR sampling on the GPU: drs_terminal_step and drs_cfg_rescale against the float64 oracle
of tests/ztsnr_oracle.py with guard bands around what they write, the chains of all three samplers, `sample_known` and the
tiler's final mode from the terminal level, the Gaussian problem with a mean, and the training step at the terminal level."""
import itertools
import math
import os
import types

import pytest
import torch

import test_gpu_prediction as TP
import ztsnr_oracle as Z
from conftest import rel_errors, replay_noise_source, replay_tile_noise
from guard import Guarded, bits_equal
from oracle import aggregation_oracle as A
from oracle import unet_oracle as U
from test_ztsnr_host import GAUSS_BOUND

pytestmark = pytest.mark.gpu

IMPL = TP.IMPL
T50 = 50
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_the_feature_is_there():
    from diffusionremotesensing_amd.hip_ops import cfg_rescale, terminal_step_  # noqa: F401 - absent before this feature
    from diffusionremotesensing_amd.sampling import rescale_zero_terminal_snr  # noqa: F401


# ---------------------------------------------------------------------------------------------
# drs_terminal_step
# ---------------------------------------------------------------------------------------------
SHAPES = {"1x1x1x1": ((1, 1, 1, 1), 0, 0), "2x3x5x7": ((2, 3, 5, 7), 0, 0), "3x2x16x20": ((3, 2, 16, 20), 0, 0),
          "2x3x5x7+1float": ((2, 3, 5, 7), 4, 4), "2x3x5x7 x alone +1float": ((2, 3, 5, 7), 4, 0)}
CLIPS = ((None, False), ((0.0, 1.0), False), ((-1.0, 1.0), False), ((0.0, 1.0), True), ((-1.0, 1.0), True))
SCALES = (0.3, 1.7, 2.5)  # per image: below both half-ranges (the static clamp), above them (the threshold)


def _guarded(t, dev, shift, what):
    g = Guarded(t.shape, t.dtype, dev, shift=shift, fill="pattern", what=what)
    g.view.copy_(t)
    return g


def _term_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, C, H, W = shape
    x, z = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    pred = torch.randn(shape, generator=g) * 0.8 + 0.3
    # |pred - pred_uncond| <= 0.1 |pred|: the guided value 3 pred - 2 pred_uncond keeps |g| >= 0.8 |pred|, so the fp32 lerp's
    # error (2^-24 (2 |d| + |g|), d = pred - pred_uncond) stays under 2^-23 |g| - the x0 term of the bound - on every element
    pu = pred * (1 + 0.1 * (2 * torch.rand(shape, generator=g) - 1))
    known = torch.rand(shape, generator=g)
    masks = {1: (torch.rand((n, 1, H, W), generator=g) < 0.4).to(torch.uint8),
             C: (torch.rand((n, C, H, W), generator=g) < 0.4).to(torch.uint8)}
    return x, z, pred, pu, known, masks


@pytest.mark.parametrize("case", list(SHAPES))
def test_terminal_step_vs_float64_oracle(dev, case):
    """Every combination of kind, clip / threshold, eta, t_prev, guidance and mask on one shape; the history on every third
    combination off.  Per element |got - want| <= 4 * 2^-24 (|c0 x0| + |c1 x| + |sigma z|) - three rounded products and two
    rounded sums on once-rounded coefficients - plus 2^-23 |x0| where guidance or the threshold formed x0 (x0: the value the
    move used and the history holds); a known pixel
    is `inpaint_step_`'s value bit for bit; the history is x0 (exactly, or within 2^-23 |x0| where fp32 arithmetic formed it);
    a second call gives the same bits; the guard bands around x and the history are intact."""
    from diffusionremotesensing_amd import hip_ops
    shape, shift, other_shift = SHAPES[case]
    n, C, H, W = shape
    ah = Z.schedule("cosine", T50)[1]
    ah_d = ah.to(dev)
    x, z, pred, pu, known, masks = _term_inputs(shape, 17)
    at = lambda t: _guarded(t, dev, other_shift, "input").view  # noqa: E731
    pred_d, pu_d, z_d, known_d = at(pred), at(pu), at(z), at(known)
    masks_d = {k: m.to(dev) for k, m in masks.items()}
    scale = torch.tensor(SCALES[:n])
    scale_d = scale.to(dev)
    worst, count = 0.0, 0
    combos = itertools.product(("v", "x0"), CLIPS, (0.0, 0.5, 1.0), (0, 23), (False, True), (None, 1, C))
    for k, (kind, (clip, dyn), eta, t_prev, guided, mc) in enumerate(combos):
        with_hist = k % 3 != 0
        need_noise = t_prev > 0 and (eta > 0 or mc is not None)
        kw = {"eta": eta, "x0_clip": clip, "scale": scale_d if dyn else None}
        if guided:
            kw.update(pred_uncond=pu_d, cfg_scale=3.0)
        if mc is not None:
            kw.update(known=known_d, known_mask=masks_d[mc])
        outs = []
        for _ in range(2):
            gx = _guarded(x, dev, shift, "x")
            gh = Guarded(shape, torch.float32, dev, shift=other_shift, fill="pattern", what="x0_hist") if with_hist else None
            hip_ops.terminal_step_(gx.view, pred_d, z_d if need_noise else None, T50 - 1, t_prev, ah_d, kind,
                                   hist=gh.view if with_hist else None, **kw)
            gx.assert_intact()
            if with_hist:
                gh.assert_intact()
            outs.append((gx.view.clone(), gh.view.clone() if with_hist else None))
        assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1]), (case, k)
        got, hist = outs[0][0].cpu(), outs[0][1].cpu() if with_hist else None
        want, x0, terms = Z.terminal_step(x, pred, z if need_noise else None, t_prev, ah, kind, eta, clip, scale if dyn else None,
                                          pu if guided else None, 3.0, known if mc is not None else None,
                                          masks[mc] if mc is not None else None)
        fp32_x0 = guided or dyn
        x0_mag = x0.abs()  # the x0 the move used and the history holds: guided, clamped or thresholded
        bound = 4 * U24 * terms + (2 * U24 * x0_mag if fp32_x0 else 0.0)
        unknown = torch.ones(shape, dtype=torch.bool) if mc is None else (masks[mc] == 0).expand(shape)
        err = (got.double() - want).abs()
        assert bool((err <= bound)[unknown].all()), (case, kind, clip, dyn, eta, t_prev, guided, mc,
                                                     (err / bound.clamp_min(1e-300))[unknown].max().item())
        if unknown.any() and bool((bound[unknown] > 0).any()):
            worst = max(worst, (err / bound.clamp_min(1e-300))[unknown & (bound > 0)].max().item())
        if mc is not None:
            # the known pixels: drs_inpaint_step's value, from any DDIM move that ends at t_prev with the same draw
            ref = x.to(dev).clone()
            hip_ops.inpaint_step_(ref, torch.zeros_like(ref), z_d.contiguous() if t_prev > 0 else None, known_d.contiguous(),
                                  masks_d[mc], T50 - 2, alpha_hat=ah_d, t_prev=t_prev, eta=eta)
            kn = ~unknown
            assert torch.equal(got[kn], ref.cpu()[kn]), (case, k)
            if t_prev == 0:
                assert torch.equal(got[kn], known[kn])
        if with_hist:
            if fp32_x0:
                assert bool(((hist.double() - x0).abs() <= 2 * U24 * x0_mag).all()), (case, k)
            else:
                assert torch.equal(hist.double(), x0), (case, k)
        count += 1
    print(f"terminal_step {case}: {count} combinations, worst error / bound {worst:.3f}")
    assert count == 2 * 5 * 3 * 2 * 2 * 3


@pytest.mark.parametrize("clip", [(0.0, 1.0), (-1.0, 1.0)], ids=["clip01", "clip-11"])
def test_terminal_step_history_under_the_threshold(dev, clip):
    """The history under the dynamic threshold equals x0 - the thresholded value it holds - within the x0 term, 2^-23 |x0|, on
    every element, next to the edges of both ranges too: a thresholded image's x0 is evaluated in fp64 and rounded once (an
    evaluation in drs_pred_to_eps_dyn's own fp32 steps misses this at clip (0, 1), where they round around 0.5: measured 700 x
    the term).  An element clamped to c +- s is lo / hi exactly.  Measured on an MI355X: worst ratio 0.498 at both clips."""
    from diffusionremotesensing_amd import hip_ops
    shape = (3, 2, 16, 20)
    ah = Z.schedule("cosine", T50)[1]
    ah_d = ah.to(dev)
    x, z, pred, pu, _, _ = _term_inputs(shape, 17)
    scale = torch.tensor(SCALES)
    worst = 0.0
    for kind, guided in itertools.product(("v", "x0"), (False, True)):
        xd, hist = x.to(dev), torch.empty(shape, device=dev)
        hip_ops.terminal_step_(xd, pred.to(dev), None, T50 - 1, 0, ah_d, kind, x0_clip=clip, scale=scale.to(dev), hist=hist,
                               **({"pred_uncond": pu.to(dev), "cfg_scale": 3.0} if guided else {}))
        x0 = Z.x0_of(kind, pred, clip, scale, pu if guided else None, 3.0)
        err = (hist.cpu().double() - x0).abs()
        assert bool((err[x0 == 0] == 0).all()) and int((x0 == clip[0]).sum()) > 0 and int((x0 == clip[1]).sum()) > 0
        worst = max(worst, (err / (2 * U24 * x0.abs()).clamp_min(1e-300)).max().item())
    print(f"terminal_step history under the threshold, clip {clip}: worst |hist - x0| / (2^-23 |x0|) = {worst:.3f}")
    assert worst <= 1.0


def test_terminal_step_planted_cases(dev):
    from diffusionremotesensing_amd import _lib, hip_ops
    shape = (2, 3, 5, 7)
    ah = Z.schedule("cosine", T50)[1].to(dev)
    x, z, pred, _, _, _ = _term_inputs(shape, 3)
    pred_d, z_d = pred.to(dev), z.to(dev)
    # a level whose alpha_hat is not 0, levels outside the table, t_prev not below t: NaN everywhere, history included
    for t, t_prev in ((T50 - 2, 5), (T50, 5), (-1, 0), (T50 + 7, 0), (T50 - 1, T50 - 1), (T50 - 1, -1), (T50 - 1, T50 + 3)):
        gx = _guarded(x, dev, 0, "x")
        gh = Guarded(shape, torch.float32, dev, fill="pattern", what="x0_hist")
        hip_ops.terminal_step_(gx.view, pred_d, z_d, t, t_prev, ah, "v", eta=0.5, hist=gh.view)
        torch.cuda.synchronize()
        gx.assert_intact()
        gh.assert_intact()
        assert bool(torch.isnan(gx.view).all()) and bool(torch.isnan(gh.view).all()), (t, t_prev)
    # an unrescaled table has no terminal level
    from oracle import diffusion_oracle as D
    xd = x.to(dev)
    hip_ops.terminal_step_(xd, pred_d, None, T50 - 1, 0, D.schedule("cosine", T50)[1].to(dev), "x0")
    assert bool(torch.isnan(xd).all())
    # an eps prediction: an error from the wrapper and from the entry point, x untouched
    xd = x.to(dev)
    with pytest.raises(ValueError, match="names no x0"):
        hip_ops.terminal_step_(xd, pred_d, None, T50 - 1, 0, ah, "eps")
    lib = _lib.load()
    st = lib.drs_terminal_step(xd.data_ptr(), pred_d.data_ptr(), None, 0.0, None, None, None, 1, 0, 0, 0.0, 0.0, None, None,
                               2, 3, 5, 7, T50 - 1, 0, 0.0, ah.data_ptr(), T50, None)
    torch.cuda.synchronize()
    assert st == 1 and b"kind" in lib.drs_last_error() and torch.equal(xd.cpu(), x)
    with pytest.raises(RuntimeError, match="noise"):
        hip_ops.terminal_step_(xd, pred_d, None, T50 - 1, 5, ah, "v", eta=0.5)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        hip_ops.terminal_step_(xd, pred_d, z_d, T50 - 1, 5, ah, "v", eta=1.5)
    with pytest.raises(RuntimeError, match="overlap"):
        hip_ops.terminal_step_(xd, pred_d, None, T50 - 1, 0, ah, "v", hist=xd)
    assert torch.equal(xd.cpu(), x)
    # a NaN or an infinity of the network is never clamped into the range
    p = pred.clone()
    p[0, 0, 0, :3] = torch.tensor([math.nan, math.inf, -math.inf])
    xd = x.to(dev)
    hip_ops.terminal_step_(xd, p.to(dev), None, T50 - 1, 0, ah, "x0", x0_clip=(0.0, 1.0))
    assert not bool(torch.isfinite(xd[0, 0, 0, :3]).any()) and bool(torch.isfinite(xd[0, 0, 0, 3:]).all())


def test_forward_jump_to_the_terminal_level_is_the_draw(dev):
    """`renoise_` up to the level whose alpha_hat is 0: r = 0, the state becomes the draw exactly."""
    from diffusionremotesensing_amd import hip_ops
    ah = Z.schedule("cosine", T50)[1].to(dev)
    g = torch.Generator().manual_seed(5)
    x, z = torch.randn((2, 3, 5, 7), generator=g).to(dev), torch.randn((2, 3, 5, 7), generator=g).to(dev)
    hip_ops.renoise_(x, z, 31, T50 - 1, ah)
    assert torch.equal(x, z)


# ---------------------------------------------------------------------------------------------
# drs_cfg_rescale
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", [1, 105, 4095, 4096, 4097])
def test_cfg_rescale_vs_float64_oracle(dev, chw):
    """n = 3 images of chw elements, the last one constant; |out - want| <= 3 * 2^-24 |want| (f rounded once, one rounded
    product, and the fp64 sums' own error), the same bits twice, guard bands around out; phi = 0 is torch.lerp, nothing else."""
    from diffusionremotesensing_amd import _lib, hip_ops
    g = torch.Generator().manual_seed(chw)
    cond, uncond = torch.randn((3, chw), generator=g) * 0.7 + 0.2, torch.randn((3, chw), generator=g)
    cond[2], uncond[2] = 0.5, 0.25  # g = 0.5 + 2 * 0.25 = 1 everywhere: std(g) == 0, f = 1
    cd, ud = cond.to(dev), uncond.to(dev)
    for phi in (0.7, 1.0):
        outs = []
        for shift in (0, 4):
            go = Guarded((3, chw), torch.float32, dev, shift=shift, fill="pattern", what="out")
            assert hip_ops.cfg_rescale(cd, ud, 3.0, phi, out=go.view) is go.view
            torch.cuda.synchronize()
            go.assert_intact()
            outs.append(go.view.clone())
        assert bits_equal(outs[0], outs[1])
        assert bits_equal(hip_ops.cfg_rescale(cd, ud, 3.0, phi), outs[0])
        want, f = Z.cfg_rescale(cond, uncond, 3.0, phi)
        err = (outs[0].cpu().double() - want).abs()
        print(f"cfg_rescale chw={chw} phi={phi}: f {f.tolist()}, worst error / |want| {(err / want.abs().clamp_min(1e-300)).max():.3e}")
        assert bool((err <= 3 * U24 * want.abs()).all())
        assert f[2].item() == 1.0 and torch.equal(outs[0][2].cpu(), torch.ones(chw))
        if chw == 1:
            assert torch.equal(outs[0].cpu(), Z.lerp32(uncond, cond, 3.0))  # one element has no spread: f = 1
        else:
            assert f[0].item() != 1.0
    # in place
    inplace = cd.clone()
    hip_ops.cfg_rescale(inplace, ud, 3.0, 0.7, out=inplace)
    assert bits_equal(inplace, hip_ops.cfg_rescale(cd, ud, 3.0, 0.7))
    # phi = 0: no launch of the library, the guided lerp of the existing path
    lib = _lib.load()
    calls = []
    counted = types.SimpleNamespace(drs_cfg_rescale=lambda *a: calls.append(a) or lib.drs_cfg_rescale(*a),
                                    drs_cfg_rescale_workspace_bytes=lib.drs_cfg_rescale_workspace_bytes,
                                    drs_last_error=lib.drs_last_error)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_lib, "_lib", counted)
        plain = hip_ops.cfg_rescale(cd, ud, 3.0, 0.0)
        assert calls == []
        hip_ops.cfg_rescale(cd, ud, 3.0, 0.5)
        assert len(calls) == 1
    assert torch.equal(plain, torch.lerp(ud, cd, 3.0)) and torch.equal(plain.cpu(), Z.lerp32(uncond, cond, 3.0))


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
# The hard cap of every family is its entry in tests/test_gpu_prediction.py's BOUNDS: a terminal move is no worse conditioned than
# the move it replaces (it divides by nothing).  Where 10 x the measured rel-L2 / the measured PSNR - 20 dB is tighter, that holds.
# Measured on an MI355X (rel-L2 / PSNR against the float64 oracle):
#   superres (16 chains)   v: 5.0e-6 .. 6.5e-6 / 108.6 .. 111.2 dB;  x0: 1.8e-5 .. 2.0e-5 / 103.4 .. 103.7 dB
#                          worst: x0, ancestral, clip (0, 1): 1.975e-5 / 103.4 dB;  v DDIM 7 threshold 0.95: 2.7e-6 / 117.5 dB
#   sar v DDIM 7, clip (-1, 1)     3.135e-6 / 111.8 dB     generation v, cfg 3, DDIM 7: phi 0: 9.157e-6 / 101.1 dB, phi 0.7: 8.094e-6 / 103.8 dB
#   sample_known v DDIM 7, resample 2, jump 2, clip (0, 1)   4.288e-6 / 112.5 dB     tiler final v DDIM 7, clip (0, 1)   5.780e-6 / 110.5 dB
#   Gaussian with a mean: DDIM 10  v 1.3e-7 / 146.3 dB, x0 1.5e-7 / 144.3 dB;  DDIM 49  v 3.380e-7 / 138.5 dB, x0 2.9e-7 / 139.8 dB
#   (against the closed form at S = 49: rel-L2 2.530e-2, the float64 chain's 2.879e-2 on its own x_T; sample mean 0.377 for MU 0.4)
MEASURED = {"superres": (1.975e-5, 103.4), "sar": (3.135e-6, 111.8), "generation": (9.157e-6, 101.1), "known": (4.288e-6, 112.5),
            "tiler": (5.780e-6, 110.5), "gauss": (3.380e-7, 138.5)}  # family -> the worst (rel-L2, PSNR) of the lines above


def _bound(family):
    cap_l2, cap_psnr = TP.BOUNDS[family]
    if family in MEASURED:
        return min(cap_l2, 10 * MEASURED[family][0]), max(cap_psnr, MEASURED[family][1] - 20)
    return cap_l2, cap_psnr


def _check_chain(family, what, got, want):
    e_max, e_l2 = rel_errors(got, want)
    psnr = TP._psnr_clamped(got, want)
    print(f"ztsnr chain {what}: max-rel {e_max:.3e} rel-L2 {e_l2:.3e} PSNR {psnr:.1f} dB (max |x| {want.abs().max():.3g})")
    assert torch.isfinite(got).all()
    l2, db = _bound(family)
    assert e_l2 <= l2 and psnr >= db, (what, e_l2, psnr)


def _sched(d):
    """The tables the chain ran on, for the oracle; they are the oracle's own."""
    got = (d.alpha.cpu(), d.alpha_hat.cpu(), d.beta.cpu())
    want = Z.schedule("cosine", d.noise_steps)
    assert torch.equal(got[1], want[1]) and got[1][-1].item() == 0.0 and got[2][-1].item() == 1.0
    return got


@pytest.fixture(scope="module")
def model(dev, seeded_sd):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    return m


def _superres(model, dev, **kw):
    return TP._superres(model, dev, T50, zero_terminal_snr=True, **kw)


@pytest.mark.parametrize("clip", [None, (0.0, 1.0)], ids=["noclip", "clip01"])
@pytest.mark.parametrize("sampler", list(TP.SAMPLERS))
@pytest.mark.parametrize("pk", ["v", "x0"])
def test_superres_chain_vs_oracle(dev, model, seeded_sd, pk, sampler, clip):
    """n = 2, 64x64 (LR 32x32, x2), rescaled cosine T = 50, the seeded weights read as a v / x0 network; the chains that draw
    nothing but x_T twice, bit for bit."""
    from diffusionremotesensing_amd import synthetic
    d = _superres(model, dev, prediction=pk, x0_clip=clip)
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    args = TP._sampling_args(TP.SAMPLERS[sampler])
    x = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
    model.eval()
    if sampler in ("ddim7_eta0", "dpmpp10"):
        again = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
        model.eval()
        assert torch.equal(x, again)
    want = Z.chain(pk, clip, Z.PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2), (2, 3, 64, 64), T50, _sched(d),
                   TP.SAMPLERS[sampler], replay_noise_source(505))
    _check_chain("superres", f"superres {pk} {sampler} clip={clip}", x, want)


def test_superres_chain_with_dynamic_threshold(dev, model, seeded_sd):
    from diffusionremotesensing_amd import synthetic
    d = _superres(model, dev, prediction="v", x0_clip=(0.0, 1.0), x0_threshold=0.95)
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    x = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(515), sampling_steps=7).cpu()
    model.eval()
    want = Z.chain("v", (0.0, 1.0), Z.PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2), (2, 3, 64, 64), T50, _sched(d),
                   ("ddim", 7, 0.0), replay_noise_source(515), threshold=0.95)
    _check_chain("superres", "superres v ddim7 clip=(0, 1) threshold 0.95", x, want)


def test_defaults_launch_what_they_launched(dev, model):
    """`zero_terminal_snr=False` and `guidance_rescale = 0.0` spelled out: the bits of a `Diffusion` built without them."""
    from diffusionremotesensing_amd import synthetic
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    outs = []
    for kw in ({}, {"zero_terminal_snr": False}):
        d = TP._superres(model, dev, T50, **kw)
        if kw:
            d.guidance_rescale = 0.0
        outs.append(d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(7), sampling_steps=7).cpu())
        model.eval()
    assert torch.equal(outs[0], outs[1])


def test_sar_v_chain_vs_oracle(dev, seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(seeded_sd_sar)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T50, device=dev, image_size=64, prediction="v",
                  x0_clip=(-1.0, 1.0), zero_terminal_snr=True)
    sar1 = synthetic.tensor_uniform("ddim.sar", (2, 64, 64))
    x = d.sample(2, m, sar1, NDVI_channels=1, noise_source=replay_noise_source(303), sampling_steps=7, eta=0.0).cpu()
    want = Z.chain("v", (-1.0, 1.0), Z.PO.sar_pred_fn(U.OracleUNetSAR(seeded_sd_sar), 2, sar1), (2, 1, 64, 64), T50, _sched(d),
                   ("ddim", 7, 0.0), replay_noise_source(303))
    _check_chain("sar", "sar v ddim7 clip=(-1, 1)", x, want)


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_generation_guided_v_chain_vs_oracle(dev, seeded_sd_gen, phi):
    """cfg_scale = 3 with guidance_rescale 0 (the guided lerp folded into the terminal move and the conversions) and 0.7 (one
    `cfg_rescale` per move first, then a single prediction everywhere)."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T50, device=dev, image_size=64, prediction="v",
                  zero_terminal_snr=True)
    d.guidance_rescale = phi
    cls = torch.tensor([2, 5])
    x = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(202),
                 sampling_steps=7, eta=0.0).cpu()
    net = U.OracleUNetGeneration(seeded_sd_gen)
    tt = lambda t: torch.full((2,), t, dtype=torch.long)  # noqa: E731
    pred_fn = Z.guided_pred_fn(lambda xs, t: net(xs, tt(t), cls), lambda xs, t: net(xs, tt(t), None), 3, phi)
    want = Z.chain("v", None, pred_fn, (2, 3, 64, 64), T50, _sched(d), ("ddim", 7, 0.0), replay_noise_source(202))
    _check_chain("generation", f"generation v cfg=3 guidance_rescale={phi} ddim7", x, want)
    if phi:
        d.guidance_rescale = 0.0
        plain = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(202),
                         sampling_steps=7, eta=0.0).cpu()
        assert not torch.equal(plain, x)  # the rescale acted


def test_sample_known_v_chain_vs_oracle(dev, model, seeded_sd):
    """Known pixels on a v chain (DDIM S = 7, eta = 0) with resample = 2 and jump = 2: the second position's resampling jumps
    back up to the terminal level and leaves it again."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.sampling import chain_moves
    d = _superres(model, dev, prediction="v", x0_clip=(0.0, 1.0))
    moves = chain_moves(T50, 7, 2, 2)
    assert sum(1 for m in moves if m.t_to == T50 - 1) == 1 and sum(1 for m in moves if m.t == T50 - 1) == 2
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    known = synthetic.tensor_uniform("prediction.known", (3, 64, 64))
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :24] = True
    x = d.sample_known(2, model, lr1, known, mask, input_channels=3, resample=2, jump=2, noise_source=replay_noise_source(606),
                       sampling_steps=7, eta=0.0).cpu()
    model.eval()
    want = Z.chain("v", (0.0, 1.0), Z.PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2), (2, 3, 64, 64), T50, _sched(d),
                   ("ddim", 7, 0.0), replay_noise_source(606), known=known, mask=mask, resample=2, jump=2)
    assert torch.equal(x[:, :, :, :24], known[None, :, :, :24].expand(2, -1, -1, -1))
    _check_chain("known", "sample_known v ddim7 resample=2 jump=2 clip=(0, 1)", x, want)


def test_tiler_final_mode_vs_oracle_and_per_step_refusal(dev, model, seeded_sd):
    """The 2 x 2-tile scene of test_gpu_prediction's tiler test: the final mode's tile chains start at the terminal level; the
    per-step mode is refused before anything runs."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    S, clip = 7, (0.0, 1.0)
    d = _superres(model, dev, prediction="v", x0_clip=clip)
    img = synthetic.tensor_uniform("prediction.scene", (1, 3, 48, 48))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(48, 48, 32, 16, 2)
    assert len(infos) == 4
    with pytest.raises(ValueError, match="per_step"):
        tiler.sample_scene(noise_source=replay_noise_source(707), sampling_steps=S, eta=0.0)
    with pytest.raises(ValueError, match="per_step"):
        tiler.aggregation_sampling(sampling_steps=S, aggregation="per_step")
    lr_tiles = torch.stack([img[0, :, y0:y0 + 32, x0:x0 + 32] for (y0, x0) in lr_origins])
    src = replay_tile_noise(808, 4, T50, (1, 3, 64, 64))
    got = tiler.sample_tiles(noise_source=src, sampling_steps=S, eta=0.0).cpu()
    model.eval()
    net, sched = U.OracleUNet(seeded_sd), _sched(d)
    want = torch.cat([Z.chain("v", clip, Z.PO.superres_pred_fn(net, 1, lr_tiles[k], 2), (1, 3, 64, 64), T50, sched,
                              ("ddim", S, 0.0), lambda i, shape, k=k: src(k, i, shape)) for k in range(4)])
    _check_chain("tiler", "tiler final v ddim7 clip=(0, 1)", got, want)


class _StubEngine:
    def check_faults(self):
        pass


@pytest.mark.parametrize("pk", ["v", "x0"])
def test_gaussian_problem_with_a_mean(dev, pk):
    """`sample_chain` with no network on per-pixel N(MU, VAR0) data: against the float64 chain on the same predictor (the
    "gauss" bound), and DDIM S = 49 against the probability-flow map MU + sqrt(VAR0) x_T within the bound the host test records
    for the float64 chain - the image's mean arrives."""
    from diffusionremotesensing_amd import sampling
    shape = (2, 3, 16, 20)
    alpha, ah, beta = Z.schedule("cosine", T50)
    pred = Z.gauss_pred(pk, ah)
    sched = types.SimpleNamespace(noise_steps=T50, alpha=alpha.to(dev), alpha_hat=ah.to(dev), beta=beta.to(dev), device=dev,
                                  prediction=pk, x0_clip=None, zero_terminal_snr=True)

    def predict(engine, x, t, first):
        return pred(x.cpu(), int(t[0].item())).to(dev).contiguous()
    for S in (10, 49):
        got = sampling.sample_chain(sched, _StubEngine(), shape, predict, table_rows=shape[0],
                                    noise_source=replay_noise_source(11), sampling_steps=S, eta=0.0).cpu()
        want = Z.chain(pk, None, pred, shape, T50, (alpha, ah, beta), ("ddim", S, 0.0), replay_noise_source(11))
        _check_chain("gauss", f"gaussian with mean {pk} ddim{S}", got, want)
    exact = Z.gauss_exact(replay_noise_source(11)(T50, shape), ah)
    err = ((got.double() - exact).norm() / exact.norm()).item()
    print(f"gaussian with mean {pk} ddim49 against the closed form: rel-L2 {err:.4e} (bound {GAUSS_BOUND:.4e}), "
          f"mean {got.mean().item():.4f} (MU {Z.MU})")
    assert err <= GAUSS_BOUND


# ---------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------
def test_train_step_at_the_terminal_level(dev, seeded_sd, tmp_path):
    """One training batch of 2 x 3 x 32 x 32 of a v network whose first image is drawn at the terminal level: that image's x_t is
    its eps and its target -x0, both exactly; the gradient handed to the UNet backward is the float64 autograd gradient of
    nn.MSELoss against that target within 2^-22 per element (test_gpu_prediction's GRAD_REL)."""
    from torch.utils.data import DataLoader
    from diffusionremotesensing_amd import hip_ops
    from diffusionremotesensing_amd.superres_feeds import SyntheticSuperresDataset
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    torch.manual_seed(1)
    torch.cuda.manual_seed(1)
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    d = Diffusion("cosine", m.to(dev), str(tmp_path / "snapshot.pt"), noise_steps=T50, device=dev, magnification_factor=2,
                  image_size=32, Degradation_type="DownBlur", prediction="v", zero_terminal_snr=True)
    d.sample_timesteps = lambda n: torch.tensor([T50 - 1, 17][:n])
    made, seen = [], {}
    noised_target, predict, nvt = d._noised_target, d._predict, hip_ops.noise_v_target

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

    def nvt_seen(x0, eps, t, alpha_hat):
        seen.setdefault("eps", []).append(eps)
        return nvt(x0, eps, t, alpha_hat)
    d._noised_target, d._predict = noised_target_seen, predict_seen
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip_ops, "noise_v_target", nvt_seen)
        d.train(lr=1e-4, epochs=1, check_preds_epoch=1, train_loader=DataLoader(SyntheticSuperresDataset(2, 3, 32, 2, seed=5), 2),
                val_loader=None, patience=10, loss="MSE", verbose=False, loss_bins=4)
    mk, eps = made[0], seen["eps"][0]
    assert mk["t"].tolist() == [T50 - 1, 17]
    assert torch.equal(mk["x_t"][0], eps[0]) and torch.equal(mk["target"][0], -mk["x0"][0])
    assert not torch.equal(mk["x_t"][1], eps[1])
    tgt = mk["target"].double()
    p = seen["pred"].double().requires_grad_()
    torch.nn.MSELoss()(p, tgt).backward()
    got, want = seen["grad"].double().cpu(), p.grad.cpu()
    zero = want == 0
    err = ((got - want).abs() / want.abs().clamp_min(1e-300))[~zero]
    print(f"train_step at the terminal level: worst relative gradient error {err.max().item():.3e} (bar {TP.GRAD_REL:.3e})")
    assert torch.isfinite(got).all() and (got[zero] == 0).all() and err.max().item() <= TP.GRAD_REL


_RUN = ["--image_size", "32", "--noise_steps", "10", "--epochs", "1", "--batch_size", "2", "--check_preds_epoch", "1", "--loss", "MSE",
        "--dataset_path", "synthetic:4", "--prediction", "v", "--zero_terminal_snr", "--guidance_rescale", "0.7",
        "--save_train_state", "--sampling_steps", "3"]


@pytest.mark.parametrize("trainer", ["superres", "sar", "generation"])
def test_trainer_command_line_with_the_flag(dev, tmp_path, monkeypatch, capsys, trainer):
    """One epoch of the trainer's command line on the rescaled schedule: it runs (its final sampling starts at the terminal
    level), writes ZERO_TERMINAL_SNR, `evaluate --zero_terminal_snr` loads the snapshot, and loading without the flag raises."""
    import importlib

    from diffusionremotesensing_amd import evaluate
    mod = importlib.import_module("diffusionremotesensing_amd." + {
        "superres": "train_diffusion_superres", "sar": "train_diffusion_SAR_TO_NDVI",
        "generation": "generate_new_imgs.train_diffusion_generation"}[trainer])
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    name = "zt_" + trainer
    argv = _RUN + ["--model_name", name] + (["--magnification_factor", "2"] if trainer == "superres" else [])
    mod.main(argv)
    weights = tmp_path / "models_run" / name / "weights"
    snap = torch.load(weights / "snapshot.pt")
    assert set(snap) == {"MODEL_STATE", "EPOCHS_RUN", "PREDICTION", "ZERO_TERMINAL_SNR"} and snap["ZERO_TERMINAL_SNR"] is True
    assert torch.load(weights / "train_state.pt")["ZERO_TERMINAL_SNR"] is True
    capsys.readouterr()
    without = [a for a in argv if a != "--zero_terminal_snr"]
    with pytest.raises(ValueError, match="zero_terminal_snr=True"):
        mod.main(without)
    if trainer == "generation":
        return  # (`evaluate` scores the two tasks that have a ground truth)
    ev = ["--model_name", name, "--image_size", "32", "--noise_steps", "10", "--batch_size", "2", "--dataset_path", "synthetic:4",
          "--sampling_steps", "3", "--prediction", "v", "--out", str(tmp_path / "r.json")]
    ev += ["--magnification_factor", "2"] if trainer == "superres" else ["--task", "sar_to_ndvi"]
    scores = evaluate.main(ev + ["--zero_terminal_snr"])
    assert scores["n"] >= 1 and all(math.isfinite(v) for v in scores["model"].values())
    with pytest.raises(ValueError, match="zero_terminal_snr=True"):
        evaluate.main(ev)
    assert os.path.exists(tmp_path / "r.json")
