"""One training step of the HIP path next to the float64 oracle's (a plain module, imported by the GPU gradient tests).

`step` runs the train-mode forward and the backward through the C-ABI on a fresh model, checks the prediction, the loss and
every BatchNorm's running statistics against the oracle and returns both gradient sets; `freeze` keeps chosen parameters
out of the backward (requires_grad False, a NULL slot in drs_unet_backward), `dout` replaces the MSE by an upstream
gradient of the caller's, `oracle` hands in an oracle_step result computed earlier (every parameter live)."""
import torch
import torch.nn.functional as F

from conftest import rel_errors
from grad_check import canonical, model_grads, oracle_step


def build_model(dev, variant, sd):
    if variant == "superres":
        from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
        m = Residual_Attention_UNet_superres(3, 3, dev)
    elif variant == "sar":
        from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
        m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    else:
        from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
        m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(sd)
    return m.to(dev).train()


def forward_args(dev, variant, x, t, cond, mag=1):
    args = (x.to(dev), t.to(dev), None if cond is None else cond.to(dev))
    return args + (mag,) if variant == "superres" else args


def check_running_stats(msd, stats, sd, tol, steps=1):
    """Running statistics of EVERY BatchNorm of the state_dict `msd` against the oracle's `stats` (both registered names of
    a ResConvBlock BatchNorm are one tensor); num_batches_tracked advanced by `steps` from `sd`.  Returns (worst, name)."""
    bns = {canonical(k)[:-len(".running_mean")] for k in msd if k.endswith(".running_mean")}
    assert bns == set(stats), sorted(bns ^ set(stats))[:8]
    worst = (0.0, "")
    for k, (rm, rv) in stats.items():
        for what, got_s, want_s in (("running_mean", msd[k + ".running_mean"], rm), ("running_var", msd[k + ".running_var"], rv)):
            e = max(rel_errors(got_s.cpu(), want_s))
            worst = max(worst, (e, f"{k}.{what}"))
            assert e <= tol, (k, what, e)
        assert int(msd[k + ".num_batches_tracked"]) == int(sd[k + ".num_batches_tracked"]) + steps, k
    return worst


def step(dev, variant, sd, x, t, cond, noise, mag=1, train_impl=None, freeze=None, dout=None, oracle=None):
    """The HIP training step and the float64 oracle's on the same batch; checks the loss and every BatchNorm's running
    statistics, returns (HIP gradients, oracle gradients).
    freeze: predicate on parameter names; those parameters get requires_grad False before the forward (their HIP gradient
            must come back None; the oracle's set stays complete).
    dout:   upstream gradient (a tensor of the prediction's shape, or a function pred -> scalar whose backward delivers
            it): replaces the MSE against `noise` on both sides; the oracle always gets the dense tensor `dout.dense`
            (function) or `dout` itself.
    oracle: an earlier oracle_step(...) result for this batch (and this dout) with every parameter live."""
    m = build_model(dev, variant, sd)
    eng = m.hip_engine()
    if train_impl is not None:
        eng.set_impl(train_impl, train_impl=train_impl)
    if freeze is not None:
        for n, p in m.named_parameters():
            if freeze(n):
                p.requires_grad_(False)
    # forward-side bars: the train-mode prediction and the running statistics of the exact-fp32 plans vs those of the
    # split-bf16 training forward (test_gpu_parity.py's train-mode bars)
    tol = 1e-3 if train_impl == "mfma_bf16x3" else 1e-4
    pred = m(*forward_args(dev, variant, x, t, cond, mag))
    if dout is None:
        loss = F.mse_loss(pred, noise.to(dev))
        loss.backward()
        dense = None
    elif callable(dout):
        loss = dout(pred)
        loss.backward()
        dense = dout.dense
    else:
        loss = (pred.detach() * dout.to(dev)).sum()
        pred.backward(dout.to(dev))
        dense = dout
    torch.cuda.synchronize()
    eng.check_faults()
    got = model_grads(m)
    if oracle is None:
        oracle = oracle_step(variant, sd, list(got), x, t, cond, noise, mag, dout=dense)
    want, ref_loss, ref, stats = oracle
    assert set(ref) == set(got), sorted(set(ref) ^ set(got))[:8]
    e_max, e_l2 = rel_errors(pred.detach().cpu(), want)
    assert e_l2 <= tol and e_max <= tol, ("prediction", e_max, e_l2)
    if dout is None:
        assert abs(loss.item() - ref_loss) <= tol * ref_loss, (loss.item(), ref_loss)
    else:  # sum(pred * dout): terms of both signs, measured against the sum of their magnitudes
        assert abs(loss.item() - ref_loss) <= tol * (want * dense.double()).abs().sum().item(), (loss.item(), ref_loss)
    worst = check_running_stats(m.state_dict(), stats, sd, tol)
    print(f"  prediction max-rel {e_max:.2e} rel-L2 {e_l2:.2e}; running statistics of {len(stats)} BatchNorms: worst {worst[0]:.2e} ({worst[1]})")
    return got, ref
