"""The frozen-BatchNorm train plan (DRS_PLAN_FROZEN_BN; model.train() with every nn.BatchNorm2d in .eval()).

Every gradient of a frozen step is compared element-wise with the float64 oracle's `training=False` autograd
(tests/frozen_step.py) at the project's bars (grad_check.REL_L2_F32 / MAX_REL_F32; REL_L2_BF16X3 for the opt-in split-bf16
plan), on weights whose running statistics are calibrated and perturbed (frozen_step.calibrated_sd) so that they are neither
trivial nor the batch's own.  The prediction is held to the bar tests/train_step.py holds the train-mode prediction to, and no
running_mean / running_var / num_batches_tracked may change a bit.  On the code before this plan existed the engine ran batch
statistics and wrote the buffers: the gradient, statistics and end-to-end tests below fail there.

A conv bias in front of a BatchNorm is no structural zero in this regime (dZ = gamma rstd g does not sum to zero): those
biases are compared like every other tensor.

Measured on MI355X (worst tensor by rel-L2): `tiny` direct 2.1e-6, mfma_f32 1.3e-5 (downs.2.weight), mfma_bf16x3 2.5e-4
(gating_signals.2.conv.weight); single-image 5.3e-5 (LR_encoder.blocks.2.conv1.bias), SAR 1.4e-5, generation 1.4e-5; `tiny` with
20 parameters frozen 1.2e-5; between guards 1.3e-5 in each mode.  Predictions 8e-7 .. 1.6e-6 (split bf16: 1.5e-5).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from frozen_step import (assert_bn_untouched, bn_buffers, calibrated_sd, frozen_model, frozen_oracle_step, frozen_step)
from grad_check import MAX_REL_F32, REL_L2_BF16X3, REL_L2_F32, check_grads, grad_scale, model_grads
from guard import MODES, bits_equal, guarded_allocations
from train_step import forward_args

pytestmark = pytest.mark.gpu

T_MAX = 1499


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _names(variant, sd):
    from train_step import build_model
    return [n for n, _ in build_model("cpu", variant, sd).named_parameters()]


def _batch(tag):
    """(variant, x, t, cond, noise, mag): test_gpu_grads' `tiny`, `single-image`, SAR and generation-with-labels batches."""
    from diffusionremotesensing_amd import synthetic
    if tag == "tiny":  # 3x5 bottleneck, partial tiles at every level, timesteps 1 and T-1
        return ("superres", synthetic.tensor_normal("grads.tiny.x", (2, 3, 24, 40)), torch.tensor([1, T_MAX]),
                synthetic.tensor_uniform("grads.tiny.lr", (2, 3, 12, 20)), synthetic.tensor_normal("grads.tiny.noise", (2, 3, 24, 40)), 2)
    if tag == "single-image":  # B = 1: what the feature exists for; levels with hh > 8 carry the SP copy of dZ; x4
        return ("superres", synthetic.tensor_normal("grads.single-image.x", (1, 3, 64, 64)), torch.tensor([1]),
                synthetic.tensor_uniform("grads.single-image.lr", (1, 3, 16, 16)),
                synthetic.tensor_normal("grads.single-image.noise", (1, 3, 64, 64)), 4)
    if tag == "sar":
        return ("sar", synthetic.tensor_normal("grads.sar.x", (2, 1, 40, 24)), torch.tensor([T_MAX, 1]),
                synthetic.tensor_uniform("grads.sar.sar", (2, 2, 40, 24)), synthetic.tensor_normal("grads.sar.noise", (2, 1, 40, 24)), 1)
    assert tag == "generation"
    return ("generation", synthetic.tensor_normal("grads.gen.x", (3, 3, 24, 40)), torch.tensor([1, 800, T_MAX]),
            torch.tensor([4, 9, 4]), synthetic.tensor_normal("grads.gen.noise", (3, 3, 24, 40)), 1)


_CASES = {}  # tag -> (calibrated state dict, batch, frozen oracle step): computed once, shared, never modified


@pytest.fixture(scope="module")
def cases(seeded_sd, seeded_sd_sar, seeded_sd_gen):
    sds = {"superres": seeded_sd, "sar": seeded_sd_sar, "generation": seeded_sd_gen}

    def get(tag):
        if tag not in _CASES:
            batch = _batch(tag)
            sd = calibrated_sd(batch[0], sds[batch[0]])
            _CASES[tag] = (sd, batch, frozen_oracle_step(batch[0], sd, _names(batch[0], sd), *batch[1:]))
        return _CASES[tag]
    return get


def _bars(impl):
    return (REL_L2_BF16X3, None) if impl == "mfma_bf16x3" else (REL_L2_F32, MAX_REL_F32)


# ---- gradients, prediction, statistics -------------------------------------------------------------------------------------
GRAD_RUNS = [("tiny", "direct"), ("tiny", "mfma_f32"), ("tiny", "mfma_bf16x3"), ("single-image", None), ("sar", None),
             ("generation", None)]


@pytest.mark.parametrize("tag,impl", GRAD_RUNS, ids=[f"{c}-{i or 'default'}" for c, i in GRAD_RUNS])
def test_frozen_grads(dev, cases, tag, impl):
    """Every gradient of the frozen step against the float64 frozen oracle; frozen_step also checks the prediction, the loss
    and that no BatchNorm buffer changed."""
    sd, batch, oracle = cases(tag)
    got, ref, _ = frozen_step(dev, batch[0], sd, *batch[1:], train_impl=impl, oracle=oracle)
    check_grads(got, ref, *_bars(impl), what=f"frozen {tag} [{impl or 'default'}]")


def test_conv_biases_in_front_of_a_batchnorm_are_live(cases):
    """In the frozen regime the oracle's gradient of such a bias is far above grad_check's structural-zero threshold, so
    check_grads compares it element-wise (in the batch-statistics regime it is skipped as a structural zero)."""
    from grad_check import ZERO_FRAC
    _, _, (_, _, ref) = cases("tiny")
    scale = grad_scale(ref)
    for name in ("conv_blocks.0.conv1.0.bias", "bottle_neck.conv2.0.bias", "ups.1.conv.bias", "gating_signals.0.conv.bias",
                 "attention_blocks.2.result.0.bias"):
        assert ref[name].norm().item() > 100 * ZERO_FRAC * scale, (name, ref[name].norm().item(), scale)


def test_frozen_forward_outside_autograd(dev, cases):
    """The train-mode forward under no_grad (what `sample` runs after its model.train(), quirk Q5) takes the frozen plan too:
    the oracle's training=False prediction at train_step's 1e-4 bar, buffers untouched, bit-equal to the autograd forward."""
    from conftest import rel_errors
    sd, batch, oracle = cases("tiny")
    variant, x, t, cond, noise, mag = batch
    m = frozen_model(dev, variant, sd)
    before = bn_buffers(m)
    with torch.no_grad():
        pred = m(*forward_args(dev, variant, x, t, cond, mag))
    torch.cuda.synchronize()
    assert m.hip_engine()._last_plan.frozen and m.hip_engine()._last_plan.train
    e_max, e_l2 = rel_errors(pred.cpu(), oracle[0])
    print(f"frozen no_grad prediction: max-rel {e_max:.2e} rel-L2 {e_l2:.2e}")
    assert e_max <= 1e-4 and e_l2 <= 1e-4
    assert_bn_untouched(m, before)
    pred2 = m(*forward_args(dev, variant, x, t, cond, mag))
    assert bits_equal(pred, pred2.detach())
    # eval mode is the folded eval plan as before, and a later train() is frozen again (sticky)
    m.eval()
    with torch.no_grad():
        m(*forward_args(dev, variant, x, t, cond, mag))
    assert not m.hip_engine()._last_plan.train
    m.train()
    with torch.no_grad():
        m(*forward_args(dev, variant, x, t, cond, mag))
    assert m.hip_engine()._last_plan.frozen
    assert_bn_untouched(m, before)


def test_default_train_step_still_updates_statistics(dev, cases):
    """The same model without freeze_batchnorm: the batch-statistics plan, whose key and behaviour are what they were."""
    sd, batch, _ = cases("tiny")
    variant, x, t, cond, noise, mag = batch
    from train_step import build_model
    m = build_model(dev, variant, sd)
    before = bn_buffers(m)
    F.mse_loss(m(*forward_args(dev, variant, x, t, cond, mag)), noise.to(dev)).backward()
    torch.cuda.synchronize()
    plan = m.hip_engine()._last_plan
    assert plan.train and not plan.frozen
    after = bn_buffers(m)
    assert all(int(after[k]) == int(before[k]) + 1 for k in before if k.endswith("num_batches_tracked"))
    assert not any(bits_equal(before[k], after[k]) for k in before if k.endswith("running_mean"))


def test_frozen_parameters_too(dev, cases):
    """freeze=("downs.", "LR_encoder.") on top of frozen BatchNorm: those parameters come back without a gradient, the others
    meet the bar, structural zeros judged against the full set's scale."""
    from diffusionremotesensing_amd.finetune import frozen_names
    sd, batch, oracle = cases("tiny")
    names = _names("superres", sd)
    from train_step import build_model
    frozen = set(frozen_names(build_model("cpu", "superres", sd), ("downs.", "LR_encoder.")))
    assert len(frozen) == 3 * 2 + 7 * 2, sorted(frozen)
    got, ref, _ = frozen_step(dev, "superres", sd, *batch[1:], freeze=lambda n: n in frozen, oracle=oracle)
    assert list(got) == names
    assert not [n for n in frozen if got[n] is not None]
    wanted = [n for n in names if n not in frozen]
    check_grads({n: got[n] for n in wanted}, {n: ref[n] for n in wanted}, REL_L2_F32, MAX_REL_F32,
                f"frozen tiny, {len(frozen)} parameters frozen", scale=grad_scale(ref))


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_mixed_batchnorm_modes_raise(dev, cases):
    sd, batch, _ = cases("tiny")
    variant, x, t, cond, noise, mag = batch
    from train_step import build_model
    m = build_model(dev, variant, sd)
    m.conv_blocks[0].batch_norm1.eval()
    before = bn_buffers(m)
    with pytest.raises(RuntimeError, match="BatchNorm2d layers are in eval mode and the others in train"):
        m(*forward_args(dev, variant, x, t, cond, mag))
    with torch.no_grad(), pytest.raises(RuntimeError, match="BatchNorm2d layers are in eval mode"):
        m(*forward_args(dev, variant, x, t, cond, mag))
    torch.cuda.synchronize()
    assert_bn_untouched(m, before)


def test_frozen_flag_needs_a_train_plan():
    """DRS_PLAN_FROZEN_BN without DRS_PLAN_TRAIN: DRS_ERR_ARG (1) and a message, with and without KEEP_ALL; with TRAIN: a plan."""
    import ctypes as C

    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    for flags in (_lib.PLAN_FROZEN_BN, _lib.PLAN_FROZEN_BN | _lib.PLAN_KEEP_ALL):
        cfg = _lib.UNetConfig(2, 2, 3, 3, 24, 40, 2, _lib.IMPL_MFMA_F32, 1e-5, flags, _lib.VARIANT_SUPERRES, 3, 0)
        h = C.c_void_p()
        assert lib.drs_unet_plan_create(C.byref(h), C.byref(cfg)) == 1
        assert b"DRS_PLAN_FROZEN_BN needs DRS_PLAN_TRAIN" in lib.drs_last_error()
        assert not h.value
    cfg = _lib.UNetConfig(2, 2, 3, 3, 24, 40, 2, _lib.IMPL_MFMA_F32, 1e-5, _lib.PLAN_FROZEN_BN | _lib.PLAN_TRAIN,
                          _lib.VARIANT_SUPERRES, 3, 0)
    h = C.c_void_p()
    assert lib.drs_unet_plan_create(C.byref(h), C.byref(cfg)) == 0 and h.value
    plain = C.c_void_p()
    cfg.flags = _lib.PLAN_TRAIN
    assert lib.drs_unet_plan_create(C.byref(plain), C.byref(cfg)) == 0
    # same workspace layout as the batch-statistics train plan
    assert lib.drs_unet_workspace_bytes(h) == lib.drs_unet_workspace_bytes(plain)
    assert lib.drs_unet_packed_bytes(h) == lib.drs_unet_packed_bytes(plain)
    lib.drs_unet_plan_destroy(h)
    lib.drs_unet_plan_destroy(plain)


def test_second_backward_still_raises(dev, cases):
    sd, batch, oracle = cases("tiny")
    variant, x, t, cond, noise, mag = batch
    m = frozen_model(dev, variant, sd)
    loss = F.mse_loss(m(*forward_args(dev, variant, x, t, cond, mag)), noise.to(dev))
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="ran twice"):
        loss.backward()
    # ... and a backward whose forward is no longer the plan's last one
    loss = F.mse_loss(m(*forward_args(dev, variant, x, t, cond, mag)), noise.to(dev))
    with torch.no_grad():
        m(*forward_args(dev, variant, x, t, cond, mag))
    with pytest.raises(RuntimeError, match="later train-mode forward"):
        loss.backward()
    m.zero_grad(set_to_none=True)
    F.mse_loss(m(*forward_args(dev, variant, x, t, cond, mag)), noise.to(dev)).backward()
    torch.cuda.synchronize()
    check_grads(model_grads(m), oracle[2], REL_L2_F32, MAX_REL_F32, "fresh frozen step after the refusals")


# ---- guard bands -----------------------------------------------------------------------------------------------------------
_NORMAL = {}


def _guard_fn(dev, sd, batch, oracle, put):
    variant = batch[0]
    m = frozen_model(dev, variant, sd)
    before = bn_buffers(m)
    x, t, cond, noise, mag = batch[1:]
    args = tuple(put(a) if isinstance(a, torch.Tensor) else a for a in forward_args(dev, variant, x, t, cond, mag))
    pred = m(*args)
    F.mse_loss(pred, put(noise.to(dev))).backward()
    torch.cuda.synchronize()
    m.hip_engine().check_faults()
    assert_bn_untouched(m, before)
    return pred.detach(), bn_buffers(m), model_grads(m)


@pytest.mark.parametrize("mode", MODES)
def test_frozen_step_between_guards(monkeypatch, dev, cases, mode):
    """The frozen `tiny` step with the workspace, the packed images, the flat gradient buffer, the weights and the inputs
    between sentinel guards, at each pointer phase: guards intact, prediction and running statistics bit-equal to the normal
    call's, gradients at the oracle bar (they are summed with float atomics: test_gpu_guard.py's EXCEPTIONS say why no two
    steps agree in their last bits)."""
    sd, batch, oracle = cases("tiny")
    if "tiny" not in _NORMAL:
        _NORMAL["tiny"] = _guard_fn(dev, sd, batch, oracle, lambda v: v)
        check_grads(_NORMAL["tiny"][2], oracle[2], REL_L2_F32, MAX_REL_F32, "frozen tiny, normal call")
    pred0, bufs0, _ = _NORMAL["tiny"]
    with guarded_allocations(monkeypatch, dev, mode) as block:
        pred, bufs, grads = _guard_fn(dev, sd, batch, oracle, block.copy)
        assert block.allocations and {"drs_unet_forward_labels", "drs_unet_backward_labels"} <= block.calls
    assert bits_equal(pred0, pred), f"[{mode}] prediction differs from the normal call"
    assert not [k for k in bufs0 if not bits_equal(bufs0[k], bufs[k])]
    check_grads(grads, oracle[2], REL_L2_F32, MAX_REL_F32, f"frozen tiny between guards [{mode}]")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_finetune_run_end_to_end(dev, tmp_path, monkeypatch, capsys, seeded_sd):
    """Diffusion.train for 2 epochs on synthetic_u8:4 (32 x 32, x2, B = 2) with freeze_bn, freeze=("LR_encoder.",) and
    init_from a snapshot written here: BatchNorm buffers and frozen parameters keep the loaded bits, other parameters move,
    the losses are finite and the snapshot the run writes loads into a fresh model."""
    import re

    from diffusionremotesensing_amd import train_diffusion_superres as T
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    monkeypatch.chdir(tmp_path)
    start = calibrated_sd("superres", seeded_sd)
    init = str(tmp_path / "pretrained.pt")
    torch.save({"MODEL_STATE": start, "EPOCHS_RUN": 37}, init)
    args = T.parse_train_args(["--image_size", "32", "--noise_steps", "10", "--epochs", "2", "--batch_size", "2",
                               "--check_preds_epoch", "1", "--loss", "MSE", "--magnification_factor", "2", "--dataset_path",
                               "synthetic_u8:4", "--Blur_radius", "0.5", "--freeze_bn", "--freeze", "LR_encoder.",
                               "--init_from", init])
    from diffusionremotesensing_amd.cli import cli_finetune
    assert cli_finetune(args) == {"freeze_bn": True, "freeze": ("LR_encoder.",), "init_from": init}
    torch.manual_seed(0)
    train_loader, val_loader, _ = T.make_superres_feeds(args, dev)
    model = Residual_Attention_UNet_superres(3, 3, dev).to(dev)
    snap = str(tmp_path / "weights" / "snapshot.pt")
    os.makedirs(os.path.dirname(snap))
    d = T.Diffusion("cosine", model, snap, noise_steps=10, device=dev, magnification_factor=2, image_size=32,
                    Degradation_type="DownBlur")
    d.train(lr=1e-3, epochs=2, check_preds_epoch=1, train_loader=train_loader, val_loader=val_loader, patience=5, loss="MSE",
            verbose=False, **cli_finetune(args))
    torch.cuda.synchronize()
    out = capsys.readouterr().out
    assert "Starting from the weights of" in out and "at Epoch 0" in out and d.epochs_run == 0
    assert "Fine-tuning: 14 parameter tensors frozen" in out and "BatchNorm statistics frozen" in out
    losses = [float(v) for v in re.findall(r"Running Train \(MSE\) ([0-9.eE+-]+|nan|inf)", out)]
    losses += [float(v) for v in re.findall(r"Running Val loss \(MSE\)([0-9.eE+-]+|nan|inf)", out)]
    assert len(losses) == 4 and all(torch.isfinite(torch.tensor(losses))), out
    now = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    buffers = [k for k in start if k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    assert len(buffers) >= 60 and not [k for k in buffers if not bits_equal(start[k], now[k])]
    frozen = [k for k in start if k.startswith("LR_encoder.")]
    assert len(frozen) == 14 and not [k for k in frozen if not bits_equal(start[k], now[k])]
    assert all(not p.requires_grad for n, p in model.named_parameters() if n.startswith("LR_encoder."))
    moved = [k for k in start if k not in buffers and k not in frozen and not bits_equal(start[k], now[k])]
    assert len(moved) > 100, len(moved)
    fresh = Residual_Attention_UNet_superres(3, 3, "cpu")
    written = torch.load(snap, map_location="cpu")
    fresh.load_state_dict(written["MODEL_STATE"])
    assert written["EPOCHS_RUN"] in (0, 1)
    assert not [k for k in buffers if not bits_equal(start[k], written["MODEL_STATE"][k])]
