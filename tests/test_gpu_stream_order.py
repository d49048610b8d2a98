"""Stream ordering of every C-ABI entry that takes a stream: the inputs arrive late, behind a spin kernel, on a stream other
than the default one (tests/late.py), and the result must be what the default stream gives.

Every case runs two default-stream baselines first.  Where they agree bit for bit (everything the code documents as free of
atomics) the late result must have the baseline's bits; otherwise it must meet the bar of the op's own GPU test.  COVERAGE
maps every entry of include/drs_hip.h that takes a `drs_stream_t` to the case that reaches it; the case asserts, through a
recording proxy of the library, that it did (tests/test_stream_order_host.py checks the table against the header).

Measured on an MI355X (host time of a warm call, the spin used, comparison group; `blocking` = the entry reads back to the
host by design and must have waited for its stream).  Spin = max(20 ms, 10 x host time):

    selftest.joined              host   0.04 ms  spin   20 ms  bit-equal
    unet.edge9                   host   0.37 ms  spin   20 ms  bit-equal
    unet.f32                     host   0.29 ms  spin   20 ms  bit-equal
    unet.gen                     host   0.43 ms  spin   20 ms  bit-equal
    unet.sar                     host   0.30 ms  spin   20 ms  bit-equal
    unet.two_calls               host   0.60 ms  spin   20 ms  bit-equal
    unet.check_faults            host   0.76 ms  spin   20 ms  bit-equal blocking
    unet.two_engines             host   0.53 ms  spin   20 ms  bit-equal
    unet.plain_abi               host   5.45 ms  spin   55 ms  tolerance
    train.batch_stats            host   7.12 ms  spin   71 ms  tolerance
    train.frozen_bn              host   6.84 ms  spin   68 ms  tolerance
    chain.ancestral              host   5.74 ms  spin   57 ms  bit-equal blocking
    chain.ddim_eta               host   3.61 ms  spin   36 ms  bit-equal blocking
    chain.dpmpp_2m               host   3.65 ms  spin   37 ms  bit-equal blocking
    chain.known_resample         host   4.72 ms  spin   47 ms  bit-equal blocking
    chain.v_threshold            host   3.81 ms  spin   38 ms  bit-equal blocking
    chain.zero_terminal_snr      host   3.78 ms  spin   38 ms  bit-equal blocking
    chain.lr_consistency         host   4.13 ms  spin   41 ms  bit-equal blocking
    chain.tiler_per_step         host   3.47 ms  spin   35 ms  bit-equal blocking
    row.adam                     host   0.16 ms  spin   20 ms  bit-equal
    row.aggregate_tiles          host   0.04 ms  spin   20 ms  bit-equal blocking
    row.aggregate_tiles_known    host   0.04 ms  spin   20 ms  bit-equal blocking
    row.upconv_fused             host   0.15 ms  spin   20 ms  bit-equal blocking
    row.vgg                      host   0.37 ms  spin   20 ms  bit-equal

The other 54 plan-less rows took 0.01 .. 0.08 ms on the host, ran behind the 20 ms spin, non-blocking, and
were bit-equal:
    add_noise_clip, bicubic_upsample, blend_step, blend_step_ddim, blend_step_dpm, blend_step_known,
    blend_step_known_ddim, bsr_blur, bsr_blur_sep, bsr_jpeg, bsr_noise, bsr_resize, bsr_sharpen, cfg_rescale,
    colorfix_adain, colorfix_wavelet, conv2d.direct, conv2d.mfma_bf16x3, conv2d.mfma_f16, conv2d.mfma_f32,
    crop_d4_pairs, crop_d4_u8, crop_d4_u8_f32, ddim_step, diffusion_loss, diffusion_loss_bins, diffusion_loss_masked,
    downblur, dpm_step, ensemble_scores, ensemble_stats, gather_pairs, gather_tiles, gather_u8, inpaint_step,
    lr_consistent_eps, metrics_pointwise, metrics_pointwise_nodata, noise_images, noise_target_nodata, noise_v_target,
    pred_to_eps, pred_to_eps_dyn, renoise, sampler_step, sampler_step_cfg, sep_apply, sep_project, ssim_mean,
    ssim_nodata, terminal_step, time_mlp, timestep_draw, x0_abs_quantile

Tolerance group (two default-stream runs differ: float atomics in the weight gradients): unet.plain_abi (gradients within
grad_check.REL_L2_F32 / MAX_REL_F32 of the default-stream run's; prediction and running statistics bit-equal), train.batch_stats
and train.frozen_bn (`_training` has the rule; measured: gradients of the late step within 5.4e-7 rel-L2 and 7.3e-7 max-rel of
the default-stream run's, parameters 1.2e-5 apart after the late step against the bar 2 lr = 6.0e-4, 5.3e-4 after six steps
against 3.6e-3).  Everything else is bit-equal.  No run was Inconclusive in three consecutive runs of the file, and in every
case - the blocking ones included - the inputs were still pending at the first library call.  The table was taken with the
harness as it stands: warm-up on a third set of values (late.warm_values), the probe at the first library call, the spin sized
by the faster of two warm calls.
"""
import contextlib
import copy
import math

import pytest
import torch

import late
from conftest import replay_noise_source
from grad_check import MAX_REL_F32, REL_L2_F32, check_grads

pytestmark = pytest.mark.gpu

T = 50  # levels of the schedule tables of the plan-less rows

# entry of include/drs_hip.h with a drs_stream_t -> the case of this file that reaches it
COVERAGE = {
    "drs_noise_images": "row.noise_images",
    "drs_sampler_step": "row.sampler_step",
    "drs_sampler_step_cfg": "row.sampler_step_cfg",
    "drs_ddim_step": "row.ddim_step",
    "drs_dpm_step": "row.dpm_step",
    "drs_inpaint_step": "row.inpaint_step",
    "drs_renoise": "row.renoise",
    "drs_noise_v_target": "row.noise_v_target",
    "drs_pred_to_eps": "row.pred_to_eps",
    "drs_x0_quantile": "row.x0_abs_quantile",
    "drs_pred_to_eps_dyn": "row.pred_to_eps_dyn",
    "drs_terminal_step": "row.terminal_step",
    "drs_cfg_rescale": "row.cfg_rescale",
    "drs_adam_multi": "row.adam",
    "drs_grad_sumsq_partials": "train.batch_stats",
    "drs_adamw_clip_multi": "train.batch_stats",
    "drs_diffusion_loss": "row.diffusion_loss",
    "drs_timestep_draw": "row.timestep_draw",
    "drs_ema_multi": "train.batch_stats",
    "drs_aggregate_tiles": "row.aggregate_tiles",
    "drs_aggregate_tiles_known": "row.aggregate_tiles_known",
    "drs_gather_tiles": "row.gather_tiles",
    "drs_blend_step": "row.blend_step",
    "drs_blend_step_ddim": "row.blend_step_ddim",
    "drs_blend_step_dpm": "row.blend_step_dpm",
    "drs_blend_step_known": "row.blend_step_known",
    "drs_metrics_pointwise": "row.metrics_pointwise",
    "drs_ssim": "row.ssim_mean",
    "drs_noise_target_nodata": "row.noise_target_nodata",
    "drs_diffusion_loss_masked": "row.diffusion_loss_masked",
    "drs_metrics_pointwise_nodata": "row.metrics_pointwise_nodata",
    "drs_ssim_nodata": "row.ssim_nodata",
    "drs_ensemble_stats": "row.ensemble_stats",
    "drs_ensemble_scores": "row.ensemble_scores",
    "drs_colorfix_wavelet": "row.colorfix_wavelet",
    "drs_colorfix_adain": "row.colorfix_adain",
    "drs_sep_apply": "row.sep_apply",
    "drs_sep_project": "row.sep_project",
    "drs_sep_project_eps": "row.lr_consistent_eps",
    "drs_downblur_u8": "row.downblur",
    "drs_add_noise_clip_f32": "row.add_noise_clip",
    "drs_gather_pairs_f32": "row.gather_pairs",
    "drs_gather_u8_f32": "row.gather_u8",
    "drs_crop_d4_u8": "row.crop_d4_u8",
    "drs_crop_d4_u8_f32": "row.crop_d4_u8_f32",
    "drs_crop_d4_pairs_f32": "row.crop_d4_pairs",
    "drs_bsr_blur": "row.bsr_blur",
    "drs_bsr_blur_sep": "row.bsr_blur_sep",
    "drs_bsr_sharpen": "row.bsr_sharpen",
    "drs_bsr_resize": "row.bsr_resize",
    "drs_bsr_noise": "row.bsr_noise",
    "drs_bsr_jpeg": "row.bsr_jpeg",
    "drs_conv2d_nchw": "row.conv2d.direct",
    "drs_upconv_fused_nchw": "row.upconv_fused",
    "drs_bicubic_upsample_nchw": "row.bicubic_upsample",
    "drs_time_mlp": "row.time_mlp",
    "drs_unet_pack_weights": "unet.edge9",
    "drs_unet_forward": "unet.plain_abi",
    "drs_unet_forward_labels": "unet.edge9",
    "drs_unet_read_tensor": "unet.sar",
    "drs_unet_backward": "unet.plain_abi",
    "drs_unet_backward_labels": "train.batch_stats",
    "drs_unet_check_faults": "unet.check_faults",
    "drs_vgg_pack_weights": "row.vgg",
    "drs_vgg_forward": "row.vgg",
    "drs_vgg_backward": "row.vgg",
    "drs_vgg_read_tensor": "row.vgg",
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    late.cycles_per_ms()  # the spin is calibrated once per module
    return torch.device("cuda:0")


@pytest.fixture()
def side(dev):
    return torch.cuda.Stream(dev)


class _Recorder:
    """The ctypes library behind a proxy that notes every drs_* function fetched for a call."""

    def __init__(self, real, calls):
        self.__dict__["_real"], self.__dict__["_calls"] = real, calls

    def __getattr__(self, name):
        if name.startswith("drs_"):
            self._calls.add(name)
            if name in COVERAGE:
                late.note_library_call()
        return getattr(self._real, name)


@contextlib.contextmanager
def _reaching(case):
    """Inside the block `_lib.load()` returns a recording proxy; on a clean exit every entry COVERAGE maps to `case` must
    have been called."""
    from diffusionremotesensing_amd import _lib
    assert case in set(COVERAGE.values()) or case in UNMAPPED_CASES, f"{case} is not a case of the coverage table"
    real_load, calls = _lib.load, set()
    _lib.load = lambda: _Recorder(real_load(), calls)
    try:
        yield calls
    finally:
        _lib.load = real_load
    missed = sorted(e for e, c in COVERAGE.items() if c == case and e not in calls)
    assert not missed, f"{case} did not reach {missed}"


def _report(case):
    rec = late.RECORDS[-1]
    print(f"[stream-order] {case}: host {rec['host_ms']:.2f} ms, spin {rec['delay_ms']:.0f} ms, {rec.get('group', '?')}"
          f"{', blocking' if rec['blocking'] else ''}")


def _rand(dev, key, shape, lo=None, hi=None):
    from diffusionremotesensing_amd import synthetic
    if lo is None:
        return synthetic.tensor_normal(f"late.{key}", shape).to(dev)
    return synthetic.tensor_uniform(f"late.{key}", shape, lo=lo, hi=hi).to(dev)


def _schedule(dev, zero_terminal=False):
    beta = torch.linspace(1e-4, 0.02, T)
    alpha = 1.0 - beta
    alpha_hat = torch.cumprod(alpha, 0)
    if zero_terminal:
        alpha_hat[T - 1] = 0.0
    return alpha.to(dev), alpha_hat.to(dev), beta.to(dev)


# =============================================================================================
# the harness itself (pure torch)
# =============================================================================================
def _selftest_inputs(dev):
    inputs = {"a": _rand(dev, "self.a", (1 << 16,)), "b": _rand(dev, "self.b", (1 << 16,))}
    return inputs, late.stale_of(inputs)


def test_harness_reports_work_on_an_unordered_stream(dev, side):
    other = torch.cuda.Stream(dev)
    inputs, stale = _selftest_inputs(dev)

    def fn(b):
        with torch.cuda.stream(other):  # no wait for the current stream
            y = b["a"] * 2 + b["b"]
        return y
    # (the baselines come from the ordered form: the unordered one races the default stream as well)
    base1 = late.baseline(lambda b: b["a"] * 2 + b["b"], inputs)
    base2 = late.baseline(lambda b: b["a"] * 2 + b["b"], inputs)
    got = late.run(fn, inputs, stale, stream=side, case="selftest.unordered", library=False)
    with pytest.raises(AssertionError, match="differs from the default-stream result"):
        late.compare(got, base1, base2, None, "selftest.unordered")


def test_harness_passes_work_forked_and_joined(dev, side):
    other = torch.cuda.Stream(dev)
    inputs, stale = _selftest_inputs(dev)

    def fn(b):
        current = torch.cuda.current_stream()
        other.wait_stream(current)
        with torch.cuda.stream(other):
            y = b["a"] * 2 + b["b"]
        current.wait_stream(other)
        return y
    _, _, group = late.check(fn, inputs, stale, stream=side, case="selftest.joined", library=False)
    assert group == "bit-equal"
    _report("selftest.joined")


def test_harness_calls_a_host_synchronisation_inconclusive(dev, side):
    inputs, stale = _selftest_inputs(dev)

    def fn(b):
        y = b["a"] * 2 + b["b"]
        torch.cuda.synchronize()
        return y
    with pytest.raises(late.Inconclusive):
        late.check(fn, inputs, stale, stream=side, case="selftest.sync", library=False)
    got, base, group = late.check(fn, inputs, stale, stream=side, blocking=True, must_sync=True, case="selftest.sync.blocking",
                                  library=False)
    assert group == "bit-equal"


# =============================================================================================
# UNet eval forward
# =============================================================================================
def _model(dev, variant, sd, impl=None, train=False):
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = {"superres": lambda: Residual_Attention_UNet_superres(3, 3, dev), "sar": lambda: Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev),
         "generation": lambda: Residual_Attention_UNet_generation(3, 3, 10, dev)}[variant]()
    m.load_state_dict(sd)
    m = m.to(dev)
    m = m.train() if train else m.eval()
    if impl is not None:
        m.hip_engine().set_impl(impl)
    return m


def _other_levels(t):
    """Another valid level per image, none equal to its true one."""
    return (t + 700) % 1499 + 1


def _superres_inputs(dev, key, B, H, W, mag=2):
    from diffusionremotesensing_amd import synthetic
    inputs = {"x": _rand(dev, f"{key}.x", (B, 3, H, W)), "t": synthetic.tensor_randint(f"late.{key}.t", (B,), 1, 1500).to(dev),
              "lr": _rand(dev, f"{key}.lr", (B, 3, H // mag, W // mag), 0.0, 1.0)}
    stale = late.stale_of(inputs, t=_other_levels(inputs["t"]))
    assert not bool((stale["t"] == inputs["t"]).any())
    return inputs, stale, {"t": (0, 1500)}


def test_unet_default_plan_edge9(dev, side, seeded_sd):
    """The default plan (split-bf16, SP, every fusion) at the `edge9` shape of test_gpu_taps.py: time MLPs, gate-bias tables and
    the composite stages' edge vectors run on the plan's side stream."""
    case = "unet.edge9"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "superres", seeded_sd, "mfma_bf16x3")
        eng = m.hip_engine()
        inputs, stale, ranges = _superres_inputs(dev, "edge9", 2, 72, 80)
        late.check(lambda b: eng.forward(b["x"], b["t"], b["lr"], 2), inputs, stale, stream=side, ranges=ranges, case=case)
        _report(case)
        _, log = eng.logged_forward(inputs["x"], inputs["t"], inputs["lr"], 2, reuse_cond=False, check_weights=False)
        eng.check_faults()
    ops, kernels = {o for o, _ in log}, {k for _, k in log}
    assert "time_mlp" in ops, sorted(ops)
    assert any("gate_bias" in k for k in kernels), sorted(kernels)
    assert any(o.endswith(".edges") for o in ops), sorted(ops)


def test_unet_fp32_plan_two_stream_decoder(dev, side, seeded_sd):
    """The exact-fp32 plan runs the attention branch of every decoder stage on the side stream."""
    case = "unet.f32"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "superres", seeded_sd, "mfma_f32")  # (the engine holds its module weakly)
        eng = m.hip_engine()
        inputs, stale, ranges = _superres_inputs(dev, "f32", 2, 24, 40)
        late.check(lambda b: eng.forward(b["x"], b["t"], b["lr"], 2), inputs, stale, stream=side, ranges=ranges, case=case)
        _report(case)
        eng.check_faults()


def test_unet_generation_labels(dev, side, seeded_sd_gen):
    from diffusionremotesensing_amd import synthetic
    case = "unet.gen"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "generation", seeded_sd_gen)
        eng = m.hip_engine()
        inputs = {"x": _rand(dev, "gen.x", (3, 3, 24, 40)), "t": synthetic.tensor_randint("late.gen.t", (3,), 1, 1500).to(dev),
                  "labels": torch.tensor([4, -1, 9], device=dev)}
        stale = late.stale_of(inputs, t=_other_levels(inputs["t"]), labels=torch.tensor([0, 0, 0], device=dev))
        late.check(lambda b: eng.forward(b["x"], b["t"], None, 1, labels=b["labels"]), inputs, stale, stream=side,
                   ranges={"t": (0, 1500), "labels": (-1, 9)}, case=case)
        _report(case)
        eng.check_faults()


def test_unet_sar(dev, side, seeded_sd_sar):
    """SAR -> NDVI, every intermediate kept: the forward and `read_tensor` behind it."""
    from diffusionremotesensing_amd import synthetic
    case = "unet.sar"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "sar", seeded_sd_sar)
        eng = m.hip_engine()
        eng.keep_intermediates = True
        inputs = {"x": _rand(dev, "sar.x", (2, 1, 40, 24)), "t": synthetic.tensor_randint("late.sar.t", (2,), 1, 1500).to(dev),
                  "sar": _rand(dev, "sar.sar", (2, 2, 40, 24), 0.0, 1.0)}
        stale = late.stale_of(inputs, t=_other_levels(inputs["t"]))

        def fn(b):
            out = eng.forward(b["x"], b["t"], b["sar"], 1)
            names = eng.tensor_names()
            return out, eng.read_tensor(names[len(names) // 2]), eng.read_tensor(names[-1])
        late.check(fn, inputs, stale, stream=side, ranges={"t": (0, 1500)}, case=case)
        _report(case)
        eng.check_faults()


def test_unet_two_calls_behind_one_delay(dev, side, seeded_sd):
    """forward(x1, t1, lr) and forward(x2, t2, lr, reuse_cond=True) on one plan behind one spin: the second call must not
    overwrite temb, the gate-bias tables or the workspace while the first still reads them."""
    from diffusionremotesensing_amd import synthetic
    case = "unet.two_calls"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "superres", seeded_sd, "mfma_bf16x3")
        eng = m.hip_engine()
        inputs, stale, ranges = _superres_inputs(dev, "two.1", 2, 72, 80)
        inputs["x2"] = _rand(dev, "two.2.x", (2, 3, 72, 80))
        inputs["t2"] = (inputs["t"] + 311) % 1499 + 1
        assert not bool((inputs["t2"] == inputs["t"]).any())
        stale = late.stale_of(inputs, t=stale["t"], t2=_other_levels(inputs["t2"]))
        ranges["t2"] = (0, 1500)

        def fn(b):
            y1 = eng.forward(b["x"], b["t"], b["lr"], 2)
            y2 = eng.forward(b["x2"], b["t2"], b["lr"], 2, reuse_cond=True)
            return y1, y2
        got, _, _ = late.check(fn, inputs, stale, stream=side, ranges=ranges, case=case)
        _report(case)
        eng.check_faults()
        # each output is its own call's: the calls one at a time, on the default stream
        alone1 = eng.forward(inputs["x"], inputs["t"], inputs["lr"], 2).clone()
        alone2 = eng.forward(inputs["x2"], inputs["t2"], inputs["lr"], 2).clone()
        torch.cuda.synchronize()
        assert late.same_bits(got[0], alone1) and late.same_bits(got[1], alone2)
        assert not torch.equal(alone1, alone2)


def test_unet_check_faults_waits_for_its_stream(dev, side, seeded_sd):
    """`check_faults()` behind a late forward: clean, the output is the baseline's, and it returns only when the work on the
    caller's stream is done (it reads the fault word back).  What `must_sync` pins here is the read-back as a whole: the copy of
    the fault word into pageable host memory already waits for the stream, so an entry whose `hipStreamSynchronize` named the
    wrong stream behaves the same (tried: such a build passes).  This is no coverage of the synchronise call itself."""
    case = "unet.check_faults"
    with _reaching(case), torch.no_grad():
        m = _model(dev, "superres", seeded_sd, "mfma_bf16x3")
        eng = m.hip_engine()
        inputs, stale, ranges = _superres_inputs(dev, "faults", 2, 24, 40)

        def fn(b):
            y = eng.forward(b["x"], b["t"], b["lr"], 2)
            eng.check_faults()
            return y
        late.check(fn, inputs, stale, stream=side, ranges=ranges, blocking=True, must_sync=True, case=case)
        _report(case)


def test_two_engines_on_two_streams(dev, seeded_sd):
    """A model and its perturbed twin, each behind its own spin on its own stream, both enqueued before either spin ends."""
    case = "unet.two_engines"
    with _reaching(case), torch.no_grad():
        m1 = _model(dev, "superres", seeded_sd, "mfma_bf16x3")
        m2 = copy.deepcopy(m1)
        m2.__dict__.pop("_hip_engine", None)
        for k, p in enumerate(m2.parameters()):
            p.mul_(1.0 + 0.01 * ((k % 5) - 2))
        engines = [m1.hip_engine(), m2.hip_engine()]
        assert engines[0] is not engines[1]
        jobs, bases = [], []
        for k, eng in enumerate(engines):
            inputs, stale, ranges = _superres_inputs(dev, f"twin.{k}", 2, 24, 40)
            fn = (lambda e: lambda b: e.forward(b["x"], b["t"], b["lr"], 2))(eng)
            bases.append((late.baseline(fn, inputs), late.baseline(fn, inputs)))
            jobs.append(late.Job(fn, inputs, stale, torch.cuda.Stream(dev), ranges))
        got = late.run_many(jobs, case=case)
        for g, (b1, b2) in zip(got, bases):
            late.compare(g, b1, b2, None, case)
        _report(case)
        assert not torch.equal(got[0], got[1])
        for eng in engines:
            eng.check_faults()


class _PlainABI:
    """The library with the `_labels` entries of the UNet routed to their plain forms (what a C caller without labels uses)."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def drs_unet_forward_labels(self, h, packed, x, t, cond, labels, nlabels, out, ws, ws_bytes, flags, stream):
        assert not labels.value and nlabels == 0
        return self._real.drs_unet_forward(h, packed, x, t, cond, out, ws, ws_bytes, flags, stream)

    def drs_unet_backward_labels(self, h, packed, packed_bwd, nbytes, x, t, labels, nlabels, dout, ptrs, ws, ws_bytes, stream):
        assert not labels.value and nlabels == 0
        return self._real.drs_unet_backward(h, packed, packed_bwd, nbytes, x, t, dout, ptrs, ws, ws_bytes, stream)


def _grads(m):
    return {n: p.grad for n, p in m.named_parameters() if p.grad is not None}


def test_unet_plain_abi_forward_backward(dev, side, seeded_sd):
    """drs_unet_forward / drs_unet_backward (no labels): one train-mode forward and backward, late batch."""
    case = "unet.plain_abi"
    with _reaching(case):
        m = _model(dev, "superres", seeded_sd, train=True)
        eng = m.hip_engine()
        inputs, stale, ranges = _superres_inputs(dev, "plain", 2, 24, 40)
        inputs["dout"] = _rand(dev, "plain.dout", (2, 3, 24, 40))
        stale["dout"] = late.nan_like(inputs["dout"])
        initial = copy.deepcopy(m.state_dict())

        def reset():
            m.load_state_dict(initial)

        def fn(b):
            for p in m.parameters():
                p.grad = None
            pred = m(b["x"], b["t"], b["lr"], 2)
            plan = eng._last_plan
            if not isinstance(plan.lib, _PlainABI):
                plan.lib = _PlainABI(plan.lib)
            pred.backward(b["dout"])
            return pred.detach(), _grads(m), dict(m.state_dict())
        # (the first forward creates the plan through the library's own entries; from then on the plain ones run)
        late.baseline(fn, inputs, reset)

        def within(got, base, _):
            # the train-mode prediction and the running statistics are repeatable; the weight gradients are added with float
            # atomics and are held to the bars of the gradient tests
            assert late.same_bits(got[0], base[0]) and late.same_bits(got[2], base[2]), late._first_difference(got[0::2], base[0::2])
            check_grads({k: v.cpu() for k, v in got[1].items()}, {k: v.cpu() for k, v in base[1].items()}, REL_L2_F32, MAX_REL_F32,
                        what=case)
        late.check(fn, inputs, stale, stream=side, ranges=ranges, case=case, reset=reset, within=within)
        _report(case)
        eng.check_faults()


# =============================================================================================
# training: forward, loss, backward, clipped AdamW, EMA
# =============================================================================================
LATE_STEPS, ALL_STEPS = 1, 6  # (a step costs the host 7 - 8 ms: one behind the spin leaves the 250 ms ceiling far away)
LR, BETAS = 3e-4, (0.9, 0.999)


def adam_travel(steps):
    """How far `steps` Adam steps can move a parameter, in units of lr: sum over k of max |m^_k| / sqrt(v^_k).  With
    m_k = (1 - b1) sum_j b1^j g_{k-j} and v_k = (1 - b2) sum_j b2^j g_{k-j}^2, Cauchy-Schwarz gives
    |m_k| <= sqrt(sum_j (1 - b1)^2 b1^(2j) / ((1 - b2) b2^j)) sqrt(v_k); the bias corrections multiply by sqrt(1 - b2^k) / (1 - b1^k).
    One step from zero moments: exactly 1 (the update is lr g / (|g| + eps))."""
    b1, b2 = BETAS
    total = 0.0
    for k in range(1, steps + 1):
        ratio = math.sqrt(sum((1 - b1) ** 2 * b1 ** (2 * j) / ((1 - b2) * b2 ** j) for j in range(k)))
        total += ratio * math.sqrt(1 - b2 ** k) / (1 - b1 ** k)
    return total


def _training(dev, side, sd, case, frozen):
    """The backward adds the weight gradients with float atomics, so two runs of the same steps differ (DESIGN.md sections 7 and
    21) and Adam turns that noise into steps of +-lr where a gradient is near zero.  Nothing here is measured against another
    noisy run.  After the late step: the loss and the running statistics, which are repeatable, have the default-stream run's
    bits; the gradients meet the bars of the gradient tests against the default-stream run's; the EMA model, which that step
    copies, has the model's bits; no parameter is further from the default-stream run's than 2 lr, what two Adam steps from the
    same state can differ by.  After all six steps everything is finite (stale inputs are NaN, and the optimizer does not skip
    a non-finite step here) and within 2 lr adam_travel(6)."""
    from diffusionremotesensing_amd.UNet_model_superres import EMA
    from diffusionremotesensing_amd.losses import DiffusionLoss
    from diffusionremotesensing_amd.optim import FusedAdamW
    m = _model(dev, "superres", sd, train=True)
    if frozen:
        m.freeze_batchnorm()
    ema_model = copy.deepcopy(m)
    ema_model.__dict__.pop("_hip_engine", None)
    initial = copy.deepcopy(m.state_dict())
    # (skip_nonfinite off: a step on stale NaN inputs must reach the parameters, not be skipped)
    opt = FusedAdamW(m.parameters(), lr=LR, betas=BETAS, weight_decay=0.01, max_grad_norm=0.5, skip_nonfinite=False)
    ema = EMA(0.995)
    loss_fn = DiffusionLoss("MSE")
    batches = []
    for k in range(ALL_STEPS):
        inputs, stale, ranges = _superres_inputs(dev, f"{case}.{k}", 2, 24, 40)
        inputs["target"] = _rand(dev, f"{case}.{k}.target", (2, 3, 24, 40))
        batches.append(inputs)
    first, first_stale = batches[0], late.stale_of(batches[0], t=_other_levels(batches[0]["t"]))
    param_names = {n for n, _ in m.named_parameters()}

    def reset():
        m.load_state_dict(initial)
        ema_model.load_state_dict(initial)
        opt.state.clear()
        ema.step = 0
        if frozen:
            m.freeze_batchnorm()

    def step(b):
        pred = m(b["x"], b["t"], b["lr"], 2)
        loss = loss_fn(pred, b["target"], b["t"])
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        ema.step_ema(ema_model, m, step_start_ema=1)  # (step 1 copies, the later ones average)
        return loss.detach()

    def state(losses):
        moments = [opt.state[p][k] for p in m.parameters() if p in opt.state for k in ("exp_avg", "exp_avg_sq")]
        return {"losses": losses, "model": dict(m.state_dict()), "ema": dict(ema_model.state_dict()), "moments": moments,
                "grads": _grads(m)}

    def fn(b):
        return state([step(b)] + [step(batches[k]) for k in range(1, LATE_STEPS)])

    def rest():
        return late._clone(state([step(batches[k]) for k in range(LATE_STEPS, ALL_STEPS)]))

    def finite(st, what):
        for part in ("losses", "moments", "model", "ema"):
            tensors = st[part].values() if isinstance(st[part], dict) else st[part]
            assert all(bool(torch.isfinite(v).all()) for v in tensors if v.is_floating_point()), f"{case}: {what}: {part} not finite"

    def apart(a, b, names):
        return max(float((a[n].double() - b[n].double()).abs().max()) for n in names)

    def within(got, base, _):
        assert late.same_bits(got["losses"], base["losses"]), (got["losses"], base["losses"])
        buffers = [n for n in got["model"] if n not in param_names]
        assert late.same_bits([got["model"][n] for n in buffers], [base["model"][n] for n in buffers]), "running statistics"
        check_grads({k: v.cpu() for k, v in got["grads"].items()}, {k: v.cpu() for k, v in base["grads"].items()}, REL_L2_F32,
                    MAX_REL_F32, what=case)
        assert late.same_bits(got["ema"], got["model"]), f"{case}: the EMA copy{late._first_difference(got['ema'], got['model'])}"
        finite(got, "after the late step")
        d, bar = apart(got["model"], base["model"], param_names), 2 * LR * adam_travel(LATE_STEPS) * (1 + 1e-3)
        print(f"  parameters after the late step: {d:.3e} from the default-stream run's (bar {bar:.3e})")
        assert d <= bar, (d, bar)

    base1 = late.baseline(fn, first, reset)
    want_all = rest()  # the ring of four pointer tables wraps here
    torch.cuda.synchronize()
    base2 = late.baseline(fn, first, reset)
    got = late.run(fn, first, first_stale, stream=side, ranges=ranges, case=case, reset=reset)
    with torch.cuda.stream(side):
        got_all = rest()
    side.synchronize()
    group = late.compare(got, base1, base2, within, case)
    if group == "bit-equal":  # (two default runs agreed to the bit: the other checks hold all the more)
        within(got, base1, None)
    _report(case)
    finite(got_all, f"after step {ALL_STEPS}")
    bar = 2 * LR * adam_travel(ALL_STEPS) * (1 + 1e-3)
    for part in ("model", "ema"):
        d = apart(got_all[part], want_all[part], param_names)
        print(f"  {part} after step {ALL_STEPS}: {d:.3e} from the default-stream run's (bar {bar:.3e})")
        assert d <= bar, (part, d, bar)
    counters = [n for n, v in got_all["model"].items() if not v.is_floating_point()]
    assert all(torch.equal(got_all["model"][n], want_all["model"][n]) for n in counters)
    assert len(got_all["moments"]) > 300
    m.hip_engine().check_faults()
    return group


def test_training_steps_batch_statistics(dev, side, seeded_sd):
    """Six training steps under a side stream, the first batch late (`_training` has what is compared).  The first step stands
    behind the spin; steps 2 .. 6 follow on the same stream (the fifth upload of the optimizer's pointer table waits for its
    ring slot's event by design, which blocks the host)."""
    with _reaching("train.batch_stats"):
        _training(dev, side, seeded_sd, "train.batch_stats", frozen=False)


def test_training_steps_frozen_batchnorm(dev, side, seeded_sd):
    with _reaching("train.frozen_bn"):
        _training(dev, side, seeded_sd, "train.frozen_bn", frozen=True)


# =============================================================================================
# sampling chains
# =============================================================================================
class _DeviceReplay:
    """`replay_noise_source(seed)` with its draws kept on the device after the first chain: later chains of the same moves
    upload nothing, so a chain's host does not wait for the device at every draw."""

    def __init__(self, seed, dev):
        self.src, self.dev, self.draws, self.k = replay_noise_source(seed), dev, [], 0

    def restart(self):
        self.k = 0
        return self

    def __call__(self, i, shape):
        if self.k == len(self.draws):
            self.draws.append(self.src(i, shape).to(self.dev))
        self.k += 1
        return self.draws[self.k - 1].clone()  # (the chain updates x_T in place)


def _diffusion(m, dev, noise_steps, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=noise_steps, device=dev, magnification_factor=2,
                     image_size=32, Degradation_type="DownBlur", **kw)


def _chain_ancestral(d, m, b, src):
    return d.sample(2, m, b["lr"], input_channels=3, noise_source=src)


def _chain_ddim(d, m, b, src):
    return d.sample(2, m, b["lr"], input_channels=3, noise_source=src, sampling_steps=5, eta=0.7)


def _chain_dpm(d, m, b, src):
    from diffusionremotesensing_amd.sampling import sampling_plan
    return d.sample(2, m, b["lr"], input_channels=3, noise_source=src, sampling_steps=sampling_plan(5, solver="dpmpp_2m"))


def _chain_known(d, m, b, src):
    return d.sample_known(2, m, b["lr"], b["known"], b["mask"], input_channels=3, resample=2, noise_source=src,
                          sampling_steps=4, eta=0.5)


def _chain_consistent(d, m, b, src):
    from diffusionremotesensing_amd.consistency import LRConsistency
    d.lr_consistency = LRConsistency()
    return d.sample(2, m, b["lr"], input_channels=3, noise_source=src, sampling_steps=5, eta=0.0)


def _chain_tiler(d, m, b, src):
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    tiler = split_aggregation_sampling(b["scene"], 16, 8, 2, d, d.device)
    assert len(tiler.patches_lr) == 4
    return tiler.aggregation_sampling(noise_source=src, sampling_steps=4, eta=0.5, aggregation="per_step")


# name: (levels, Diffusion keywords, the chain, which inputs it takes)
CHAINS = {
    "ancestral": (10, {}, _chain_ancestral, ("lr",)),
    "ddim_eta": (20, {}, _chain_ddim, ("lr",)),
    "dpmpp_2m": (20, {}, _chain_dpm, ("lr",)),
    "known_resample": (20, {}, _chain_known, ("lr", "known", "mask")),
    "v_threshold": (20, {"prediction": "v", "x0_clip": (0.0, 1.0), "x0_threshold": 0.9}, _chain_ddim, ("lr",)),
    "zero_terminal_snr": (20, {"prediction": "v", "zero_terminal_snr": True}, _chain_ddim, ("lr",)),
    "lr_consistency": (20, {}, _chain_consistent, ("lr",)),
    "tiler_per_step": (20, {}, _chain_tiler, ("scene",)),
}
UNMAPPED_CASES = {"unet.f32", "unet.gen", "unet.two_calls", "unet.two_engines", "train.frozen_bn", "row.conv2d.mfma_f32",
                  "row.conv2d.mfma_bf16x3", "row.conv2d.mfma_f16", "row.diffusion_loss_bins",
                  "row.blend_step_known_ddim"} | {f"chain.{k}" for k in CHAINS}


@pytest.mark.parametrize("name", list(CHAINS))
def test_sampling_chain(dev, side, seeded_sd, name):
    """One reverse chain per move family under a side stream, replayed noise, the conditioning image late.  blocking: every
    chain ends by reading the fault word back."""
    case = f"chain.{name}"
    levels, kw, chain, takes = CHAINS[name]
    with _reaching(case):
        m = _model(dev, "superres", seeded_sd)
        d = _diffusion(m, dev, levels, **kw)
        src = _DeviceReplay(1234, dev)
        every = {"lr": _rand(dev, f"{case}.lr", (2, 3, 16, 16), 0.0, 1.0), "scene": _rand(dev, f"{case}.scene", (1, 3, 24, 24), 0.0, 1.0),
                 "known": _rand(dev, f"{case}.known", (3, 32, 32), 0.0, 1.0),
                 "mask": (_rand(dev, f"{case}.mask", (32, 32), 0.0, 1.0) < 0.4).to(torch.uint8)}
        inputs = {k: every[k] for k in takes}
        stale = late.stale_of(inputs, **({"mask": 1 - every["mask"]} if "mask" in takes else {}))

        def fn(b):
            m.eval()
            return chain(d, m, b, src.restart())
        got, base, _ = late.check(fn, inputs, stale, stream=side, ranges={"mask": (0, 1)} if "mask" in takes else None,
                                  blocking=True, case=case)
        _report(case)
        assert bool(torch.isfinite(got).all())


# =============================================================================================
# plan-less entries
# =============================================================================================
def _row(fn, inputs, stale=None, ranges=None, blocking=False, must_sync=False, within=None, reset=None):
    return {"fn": fn, "inputs": inputs, "stale": late.stale_of(inputs, **(stale or {})), "ranges": ranges, "blocking": blocking,
            "must_sync": must_sync, "within": within, "reset": reset}


def _levels(dev, key, n, lo=1):
    from diffusionremotesensing_amd import synthetic
    t = synthetic.tensor_randint(f"late.{key}.t", (n,), lo, T).to(dev)
    return t, (t + 17) % (T - lo) + lo


def _step_inputs(dev, key, shape=(2, 3, 16, 20), names=("x", "eps", "noise")):
    return {n: _rand(dev, f"{key}.{n}", shape) for n in names}


def _rows_reverse(dev):
    from diffusionremotesensing_amd import hip_ops as H
    alpha, ah, beta = _schedule(dev)
    _, ah_z, _ = _schedule(dev, zero_terminal=True)
    rows = {}
    rows["sampler_step"] = _row(lambda b: H.sampler_step_(b["x"], b["eps"], b["noise"], 31, alpha, ah, beta), _step_inputs(dev, "ss"))
    rows["sampler_step_cfg"] = _row(lambda b: H.sampler_step_cfg_(b["x"], b["eps"], b["unc"], 3.0, b["noise"], 31, alpha, ah, beta),
                                    _step_inputs(dev, "ssc", names=("x", "eps", "unc", "noise")))
    rows["ddim_step"] = _row(lambda b: H.ddim_step_(b["x"], b["eps"], b["noise"], 31, 20, 0.5, ah, eps_uncond=b["unc"], cfg_scale=3.0),
                             _step_inputs(dev, "ddim", names=("x", "eps", "unc", "noise")))
    rows["dpm_step"] = _row(lambda b: (H.dpm_step_(b["x"], b["eps"], b["hist"], 40, 31, 20, ah), b["hist"]),
                            _step_inputs(dev, "dpm", names=("x", "eps", "hist")))
    mask = (_rand(dev, "inp.mask", (2, 1, 16, 20), 0.0, 1.0) < 0.4).to(torch.uint8)
    known = dict(_step_inputs(dev, "inp", names=("x", "eps", "noise", "known")), mask=mask)
    rows["inpaint_step"] = _row(lambda b: H.inpaint_step_(b["x"], b["eps"], b["noise"], b["known"], b["mask"], 31, alpha_hat=ah,
                                                          alpha=alpha, beta=beta), known, {"mask": 1 - mask}, {"mask": (0, 1)})
    rows["renoise"] = _row(lambda b: H.renoise_(b["x"], b["noise"], 12, 31, ah), _step_inputs(dev, "ren", names=("x", "noise")))
    t, t_stale = _levels(dev, "ni", 2)
    rows["noise_images"] = _row(lambda b: H.noise_images(b["x"], b["eps"], b["t"], ah), dict(_step_inputs(dev, "ni", names=("x", "eps")), t=t),
                                {"t": t_stale}, {"t": (0, T - 1)})
    rows["noise_v_target"] = _row(lambda b: H.noise_v_target(b["x"], b["eps"], b["t"], ah),
                                  dict(_step_inputs(dev, "nv", names=("x", "eps")), t=t), {"t": t_stale}, {"t": (0, T - 1)})
    x0 = _rand(dev, "nd.x0", (2, 3, 16, 20), 0.0, 1.0)
    x0[0, 1, 3:9, 4:11] = float("nan")
    rows["noise_target_nodata"] = _row(lambda b: H.noise_target_nodata(b["x0"], b["eps"], b["t"], ah, "v", True),
                                       {"x0": x0, "eps": _rand(dev, "nd.eps", (2, 3, 16, 20)), "t": t}, {"t": t_stale}, {"t": (0, T - 1)})
    pred = dict(_step_inputs(dev, "p2e", names=("pred", "x", "unc")), t=t)
    rows["pred_to_eps"] = _row(lambda b: H.pred_to_eps_(b["pred"], b["x"], b["t"], ah, "v", (-1.0, 1.0), pred_uncond=b["unc"], cfg_scale=3.0),
                               pred, {"t": t_stale}, {"t": (0, T - 1)})

    def dyn(b):
        scale = torch.empty(2, dtype=torch.float32, device=dev)
        out = torch.empty_like(b["pred"])
        H.pred_to_eps_(b["pred"], b["x"], b["t"], ah, "v", (-1.0, 1.0), pred_uncond=b["unc"], cfg_scale=3.0, out=out, x0_threshold=0.9,
                       scale_out=scale)
        return out, scale
    rows["pred_to_eps_dyn"] = _row(dyn, pred, {"t": t_stale}, {"t": (0, T - 1)})
    rows["x0_abs_quantile"] = _row(lambda b: H.x0_abs_quantile(b["pred"], b["x"], b["t"], ah, "v", (-1.0, 1.0), 0.9, pred_uncond=b["unc"],
                                                               cfg_scale=3.0), pred, {"t": t_stale}, {"t": (0, T - 1)})
    term = dict(_step_inputs(dev, "term", names=("x", "pred", "noise", "known", "hist")), mask=mask,
                scale=_rand(dev, "term.scale", (2,), 0.3, 2.5))
    rows["terminal_step"] = _row(lambda b: (H.terminal_step_(b["x"], b["pred"], b["noise"], T - 1, 31, ah_z, "v", eta=0.5, x0_clip=(-1.0, 1.0),
                                                             scale=b["scale"], known=b["known"], known_mask=b["mask"], hist=b["hist"]),
                                            b["hist"]), term, {"mask": 1 - mask}, {"mask": (0, 1)})
    rows["cfg_rescale"] = _row(lambda b: H.cfg_rescale(b["cond"], b["unc"], 3.0, 0.7), _step_inputs(dev, "cfgr", (3, 3, 37, 41), ("cond", "unc")))
    return rows


def _rows_tiles(dev):
    from diffusionremotesensing_amd import hip_ops as H
    alpha, ah, beta = _schedule(dev)
    S, Hs, Ws = 16, 24, 24
    origins = [(0, 0), (0, 8), (8, 0), (8, 8)]
    yy = torch.arange(S, dtype=torch.float32) - (S - 1) / 2
    weight = torch.exp(-(yy[:, None] ** 2 + yy[None, :] ** 2) / (2 * 4.0 ** 2)).to(dev).contiguous()
    table = H.tile_origins(origins, S, Hs, Ws, dev)
    table_stale = H.tile_origins([(8, 8), (8, 0), (0, 8), (0, 0)], S, Hs, Ws, dev)
    mask = (_rand(dev, "tile.mask", (1, Hs, Ws), 0.0, 1.0) < 0.4).to(torch.uint8)
    tiles = _rand(dev, "tile.tiles", (4, 3, S, S), 0.0, 1.0)
    known = _rand(dev, "tile.known", (3, Hs, Ws), 0.0, 1.0)
    rows = {}
    rows["aggregate_tiles"] = _row(lambda b: H.aggregate_tiles(b["tiles"], origins, weight, Hs, Ws), {"tiles": tiles}, blocking=True,
                                   must_sync=True)
    rows["aggregate_tiles_known"] = _row(lambda b: H.aggregate_tiles(b["tiles"], origins, weight, Hs, Ws, clamp=(0.1, 0.9), known=b["known"],
                                                                     known_mask=b["mask"]),
                                         {"tiles": tiles, "known": known, "mask": mask}, {"mask": 1 - mask}, {"mask": (0, 1)}, blocking=True,
                                         must_sync=True)
    scene = {"scene": _rand(dev, "tile.scene", (3, Hs, Ws)), "origins": table}
    rows["gather_tiles"] = _row(lambda b: H.gather_tiles(b["scene"], b["origins"], S), scene, {"origins": table_stale},
                                {"origins": (0, Hs - S)})
    blend = {"scene": scene["scene"], "eps": _rand(dev, "tile.eps", (4, 3, S, S)), "noise": _rand(dev, "tile.noise", (3, Hs, Ws)),
             "origins": table}
    org = ({"origins": table_stale}, {"origins": (0, Hs - S)})

    def counted(step):
        def fn(b):
            uncovered = torch.zeros(1, dtype=torch.int32, device=dev)
            return step(b, uncovered), uncovered
        return fn
    rows["blend_step"] = _row(counted(lambda b, u: H.blend_step_(b["scene"], b["eps"], b["origins"], weight, b["noise"], 31, alpha_hat=ah,
                                                                 alpha=alpha, beta=beta, uncovered=u)), blend, *org)
    rows["blend_step_ddim"] = _row(counted(lambda b, u: H.blend_step_(b["scene"], b["eps"], b["origins"], weight, b["noise"], 31, alpha_hat=ah,
                                                                      t_prev=20, eta=0.5, uncovered=u)), blend, *org)
    dpm = {k: v for k, v in blend.items() if k != "noise"}
    dpm["hist"] = _rand(dev, "tile.hist", (3, Hs, Ws))
    rows["blend_step_dpm"] = _row(counted(lambda b, u: (H.blend_step_(b["scene"], b["eps"], b["origins"], weight, None, 31, alpha_hat=ah,
                                                                      t_prev=20, hist=b["hist"], t_q=40, uncovered=u), b["hist"])), dpm, *org)
    # known pixels: the ancestral and the DDIM form; `blend_step_` refuses them on a DPM-Solver++(2M) move (no such entry)
    kn = dict(blend, known=known, mask=mask)
    kn_stale, kn_ranges = {"origins": table_stale, "mask": 1 - mask}, {"origins": (0, Hs - S), "mask": (0, 1)}
    rows["blend_step_known"] = _row(counted(lambda b, u: H.blend_step_(b["scene"], b["eps"], b["origins"], weight, b["noise"], 31,
                                                                       alpha_hat=ah, alpha=alpha, beta=beta, uncovered=u, known=b["known"],
                                                                       known_mask=b["mask"])), kn, kn_stale, kn_ranges)
    rows["blend_step_known_ddim"] = _row(counted(lambda b, u: H.blend_step_(b["scene"], b["eps"], b["origins"], weight, b["noise"], 31,
                                                                            alpha_hat=ah, t_prev=20, eta=0.5, uncovered=u, known=b["known"],
                                                                            known_mask=b["mask"])), kn, kn_stale, kn_ranges)
    return rows


def _rows_scores(dev):
    from diffusionremotesensing_amd import hip_ops as H
    from diffusionremotesensing_amd.consistency import SeparableOperator
    pair = {"sr": _rand(dev, "met.sr", (2, 3, 19, 23), -0.1, 1.1), "hr": _rand(dev, "met.hr", (2, 3, 19, 23), 0.0, 1.0)}
    holes = dict(pair, hr=pair["hr"].clone())
    holes["hr"][1, :, 2:5, 3:9] = float("nan")
    rows = {}
    rows["metrics_pointwise"] = _row(lambda b: H.metrics_pointwise(b["sr"], b["hr"]), pair)
    rows["ssim_mean"] = _row(lambda b: H.ssim_mean(b["sr"], b["hr"]), pair)
    rows["metrics_pointwise_nodata"] = _row(lambda b: H.metrics_pointwise_nodata(b["sr"], b["hr"], True), holes)
    rows["ssim_nodata"] = _row(lambda b: H.ssim_nodata(b["sr"], b["hr"], True), holes)
    members = {"members": _rand(dev, "ens.m", (5, 2, 3, 9, 11), 0.0, 1.0), "truth": _rand(dev, "ens.t", (2, 3, 9, 11), 0.0, 1.0)}
    rows["ensemble_stats"] = _row(lambda b: H.ensemble_stats(b["members"], quantiles=[0.1, 0.5, 0.9], clamp=(0.0, 1.0)),
                                  {"members": members["members"]})
    rows["ensemble_scores"] = _row(lambda b: H.ensemble_scores(b["members"], b["truth"], crps_map=True), members)
    color = {"sr": _rand(dev, "col.sr", (2, 3, 70, 66), 0.0, 1.0), "guide": _rand(dev, "col.g", (2, 3, 70, 66), 0.0, 1.0)}
    rows["colorfix_wavelet"] = _row(lambda b: H.colorfix_wavelet(b["sr"], b["guide"]), color)
    rows["colorfix_adain"] = _row(lambda b: H.colorfix_adain(b["sr"], b["guide"]), color)
    projector = SeparableOperator.downblur((24, 24), 2, 0.5).projector(0.01, dev)
    _, ah, _ = _schedule(dev)
    x = _rand(dev, "sep.x", (2, 3, 24, 24))
    y = _rand(dev, "sep.y", (2, 3, 12, 12), 0.0, 1.0)
    rows["sep_apply"] = _row(lambda b: H.sep_apply(b["x"], projector.D_y, projector.D_x), {"x": x})
    rows["sep_project"] = _row(lambda b: H.sep_project(b["x"], projector.prepare(b["y"]), projector, 0.8), {"x": x, "y": y})
    t, t_stale = _levels(dev, "sep", 2)
    rows["lr_consistent_eps"] = _row(lambda b: H.lr_consistent_eps_(b["eps"], b["x"], b["t"], ah, projector.prepare(b["y"]), projector, 0.8),
                                     {"eps": _rand(dev, "sep.eps", (2, 3, 24, 24)), "x": x, "y": y, "t": t}, {"t": t_stale}, {"t": (0, T - 1)})
    return rows


def _rows_layers(dev):
    from diffusionremotesensing_amd import hip_ops as H
    rows = {}
    rows["bicubic_upsample"] = _row(lambda b: H.bicubic_upsample(b["x"], 2), {"x": _rand(dev, "bic.x", (2, 3, 9, 13))})
    mlp = [_rand(dev, f"mlp.{k}", s) * 0.1 for k, s in (("W1", (256, 100)), ("b1", (256,)), ("W2", (256, 256)), ("b2", (256,)))]
    t, t_stale = _levels(dev, "mlp", 3)
    rows["time_mlp"] = _row(lambda b: H.time_mlp(b["t"], *mlp), {"t": t}, {"t": t_stale}, {"t": (0, 1500)})
    w, bias = _rand(dev, "conv.w", (32, 16, 3, 3)) * 0.08, _rand(dev, "conv.b", (32,)) * 0.1
    for impl in ("direct", "mfma_f32", "mfma_bf16x3", "mfma_f16"):
        rows[f"conv2d.{impl}"] = _row((lambda i: lambda b: H.conv2d(b["x"], w, bias, padding=1, relu=True, impl=i))(impl),
                                      {"x": _rand(dev, "conv.x", (2, 16, 16, 16))})
    N, Cc, Ch, LH, LW = 3, 32, 32, 9, 17
    up = [_rand(dev, "up.tw", (Cc, Cc, 3, 3)) * 0.1, _rand(dev, "up.tb", (Cc,)) * 0.3, _rand(dev, "up.vw", (Ch, Cc + Ch, 3, 3)) * 0.04,
          _rand(dev, "up.vb", (Ch,)) * 0.3]
    # (the entry reads its kernels' fault word back: it has waited for its stream when it returns)
    rows["upconv_fused"] = _row(lambda b: H.upconv_fused(b["h"], b["att"], *up, post2=b["post2"]),
                                {"h": _rand(dev, "up.h", (N, Cc, LH, LW)), "att": _rand(dev, "up.att", (N, Ch, 2 * LH, 2 * LW)),
                                 "post2": _rand(dev, "up.p2", (N, Ch))}, blocking=True, must_sync=True)
    return rows


def _rows_training(dev):
    from diffusionremotesensing_amd.losses import DiffusionLoss, LossAwareSampler, LossBins
    from diffusionremotesensing_amd.optim import FusedAdam
    from diffusionremotesensing_amd.perceptual import VGGPerceptualLoss
    import vgg_oracle
    rows = {}
    shape = (3, 3, 17, 241)
    t, t_stale = _levels(dev, "loss", 3, lo=0)
    table = _rand(dev, "loss.table", (T,), 0.05, 1.05)
    valid = (_rand(dev, "loss.valid", (3, 1, 17, 241), 0.0, 1.0) < 0.7).to(torch.uint8)
    data = {"pred": _rand(dev, "loss.pred", shape), "target": _rand(dev, "loss.target", shape), "t": t,
            "w": _rand(dev, "loss.w", (3,), 0.5, 2.0)}

    def loss_row(masked, with_bins, kind):
        def fn(b):
            bins = LossBins(T, 5, dev, history=4) if with_bins else None
            loss_fn = DiffusionLoss(kind, table=table, bins=bins)
            for _ in range(2 if with_bins else 1):  # (the second call appends behind the first in every ring)
                loss, grad = loss_fn.loss_and_grad(b["pred"], b["target"], b["t"], b["w"], valid=b["valid"] if masked else None)
            return loss, grad, loss_fn.per_image, loss_fn.loss_f64, loss_fn.valid_counts, None if bins is None else bins.buf
        return fn
    rows["diffusion_loss"] = _row(loss_row(False, False, "Huber"), data, {"t": t_stale}, {"t": (0, T - 1)})
    rows["diffusion_loss_bins"] = _row(loss_row(False, True, "MSE"), data, {"t": t_stale}, {"t": (0, T - 1)})
    rows["diffusion_loss_masked"] = _row(loss_row(True, True, "MSE"), dict(data, valid=valid), {"t": t_stale, "valid": 1 - valid},
                                         {"t": (0, T - 1), "valid": (0, 1)})
    bins = LossBins(T, 5, dev, history=4)
    full = DiffusionLoss("MSE", bins=bins)
    for k in range(8):  # every ring full: the draw is loss-aware
        full.loss_and_grad(_rand(dev, f"draw.p{k}", (10, 1, 8, 8)) * (1 + k), _rand(dev, f"draw.q{k}", (10, 1, 8, 8)),
                           torch.arange(10, device=dev) * 5 + k % 5)
    sampler = LossAwareSampler(bins, 0.01)
    rows["timestep_draw"] = _row(lambda b: sampler.draw(33, b["u"]), {"u": _rand(dev, "draw.u", (2, 33), 0.0, 1.0)})

    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in ((7, 5), (4097,), (3, 3, 3, 3))]
    opt = FusedAdam(params, lr=1e-2)
    adam = {}
    for k, p in enumerate(params):
        adam[f"p{k}"], adam[f"g{k}"] = _rand(dev, f"adam.p{k}", tuple(p.shape)), _rand(dev, f"adam.g{k}", tuple(p.shape))

    def adam_fn(b):
        opt.state.clear()
        with torch.no_grad():
            for k, p in enumerate(params):
                p.copy_(b[f"p{k}"])
        for _ in range(2):
            for k, p in enumerate(params):
                p.grad = b[f"g{k}"]
            opt.step()
        return [p.detach() for p in params], [opt.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")]
    rows["adam"] = _row(adam_fn, adam)

    vgg = VGGPerceptualLoss(dev, state_dict=vgg_oracle.seeded_vgg_state_dict())

    def vgg_fn(b):
        pred = b["pred"].detach().requires_grad_(True)
        loss = vgg(pred, b["target"])
        loss.backward()
        plan = vgg._plan(1, 64, 64)
        return loss.detach(), pred.grad, plan.read_tensor("features")
    rows["vgg"] = _row(vgg_fn, {"pred": _rand(dev, "vgg.pred", (1, 3, 64, 64)), "target": _rand(dev, "vgg.target", (1, 3, 64, 64))})
    return rows


def _rows_feeds(dev):
    from diffusionremotesensing_amd import augment, bsr, degradation, feeds
    rows = {}

    def u8(key, shape):
        return (_rand(dev, key, shape, 0.0, 256.0)).clamp(0, 255).to(torch.uint8)
    hr = u8("feed.hr", (2, 3, 32, 40))
    rows["downblur"] = _row(lambda b: degradation.downblur(b["hr"], 2, 0.5), {"hr": hr}, {"hr": 255 - hr}, {"hr": (0, 255)})
    rows["add_noise_clip"] = _row(lambda b: degradation.add_noise_clip_(b["x"], b["noise"]),
                                  {"x": _rand(dev, "anc.x", (2, 3, 9, 13), 0.0, 1.0), "noise": _rand(dev, "anc.n", (2, 9, 13, 3)) * 0.1})
    L = 5
    sar, ndvi = _rand(dev, "feed.sar", (L, 2, 9, 9)), _rand(dev, "feed.ndvi", (L, 1, 9, 9))
    idx, idx_stale = torch.tensor([2, 1, 2, 4, 0], device=dev), torch.tensor([0, 3, 1, 0, 4], device=dev)
    cache, labels = u8("feed.u8", (L, 3, 9, 9)), torch.tensor([3, 1, 4, 1, 5], device=dev)
    rows["gather_pairs"] = _row(lambda b: feeds.gather_pairs(b["sar"], b["ndvi"], b["idx"]), {"sar": sar, "ndvi": ndvi, "idx": idx},
                                {"idx": idx_stale}, {"idx": (0, L - 1)})
    rows["gather_u8"] = _row(lambda b: feeds.gather_u8(b["cache"], b["labels"], b["idx"]), {"cache": cache, "labels": labels, "idx": idx},
                             {"cache": 255 - cache, "labels": 9 - labels, "idx": idx_stale},
                             {"cache": (0, 255), "labels": (0, 9), "idx": (0, L - 1)})
    # (src, y0, x0, code): windows of 7 x 7 inside 9 x 9, all eight dihedral codes
    items = torch.tensor([[0, 0, 0, 0], [4, 2, 2, 7], [2, 1, 0, 3], [3, 0, 2, 5], [1, 2, 1, 6]], dtype=torch.int32, device=dev)
    items_stale = torch.tensor([[4, 2, 2, 1], [0, 0, 0, 2], [1, 0, 1, 4], [2, 2, 0, 0], [3, 1, 2, 3]], dtype=torch.int32, device=dev)
    it = ({"items": items_stale}, {"items": (0, 7)})
    rows["crop_d4_u8"] = _row(lambda b: augment.crop_d4_u8(b["cache"], b["items"], 7), {"cache": cache, "items": items},
                              {"cache": 255 - cache, **it[0]}, {"cache": (0, 255), **it[1]})
    rows["crop_d4_u8_f32"] = _row(lambda b: augment.crop_d4_u8_f32(b["cache"], b["labels"], b["items"], 7),
                                  {"cache": cache, "labels": labels, "items": items},
                                  {"cache": 255 - cache, "labels": 9 - labels, **it[0]}, {"cache": (0, 255), "labels": (0, 9), **it[1]})
    rows["crop_d4_pairs"] = _row(lambda b: augment.crop_d4_pairs(b["sar"], b["ndvi"], b["items"], 7), {"sar": sar, "ndvi": ndvi, "items": items},
                                 *it)
    x = _rand(dev, "bsr.x", (2, 3, 24, 40), 0.0, 1.0)
    kernels = torch.stack([torch.from_numpy(bsr.isotropic_gaussian(7, s)).float() for s in (0.8, 1.7)]).to(dev).contiguous()
    rows["bsr_blur"] = _row(lambda b: bsr.blur(b["x"], b["k"]), {"x": x, "k": kernels})
    rows["bsr_blur_sep"] = _row(lambda b: bsr.blur_sep(b["x"], bsr.usm_taps(9)), {"x": x})
    rows["bsr_sharpen"] = _row(lambda b: bsr.sharpen(b["x"]), {"x": x})
    rows["bsr_resize"] = _row(lambda b: bsr.resize(b["x"], 13, 21, 2, quantise=True), {"x": x})
    mode = torch.tensor([[0, 0], [0, 1]], dtype=torch.int32, device=dev)
    par = torch.zeros(2, 10, device=dev)
    par[:, 0] = 0.05
    par[:, 1], par[:, 5], par[:, 9] = 1.0, 1.0, 1.0
    rows["bsr_noise"] = _row(lambda b: bsr.noise_(b["x"], b["z"], mode, par), {"x": x, "z": _rand(dev, "bsr.z", (2, 3, 24, 40))})
    quality = torch.tensor([35, 90], dtype=torch.int32, device=dev)
    rows["bsr_jpeg"] = _row(lambda b: bsr.jpeg(b["x"], b["q"]), {"x": x, "q": quality},
                            {"q": torch.tensor([80, 40], dtype=torch.int32, device=dev)}, {"q": (1, 100)})
    return rows


_BUILDERS = (_rows_reverse, _rows_tiles, _rows_scores, _rows_layers, _rows_training, _rows_feeds)
ROW_NAMES = sorted({c[4:] for c in set(COVERAGE.values()) | UNMAPPED_CASES if c.startswith("row.")})
_ROWS = {}


def _rows(dev):
    if not _ROWS:
        for build in _BUILDERS:
            for name, row in build(dev).items():
                assert name not in _ROWS, name
                _ROWS[name] = row
    return _ROWS


def test_the_row_table_is_the_coverage_tables(dev):
    assert sorted(_rows(dev)) == ROW_NAMES, sorted(set(_rows(dev)) ^ set(ROW_NAMES))


@pytest.mark.parametrize("name", ROW_NAMES)
def test_plan_less_entry(dev, side, name):
    """One row per wrapper: every tensor input late.  blocking=False pins "no host synchronisation"; the rows that return host
    values or read a fault word back are blocking and must have waited for their stream."""
    case = f"row.{name}"
    with _reaching(case):
        row = _rows(dev)[name]
        late.check(row["fn"], row["inputs"], row["stale"], stream=side, ranges=row["ranges"], blocking=row["blocking"],
                   must_sync=row["must_sync"], within=row["within"], reset=row["reset"], case=case)
        _report(case)
