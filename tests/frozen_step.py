"""One frozen-BatchNorm training step of the HIP path next to the float64 oracle's (a plain module beside train_step.py,
imported by tests/test_gpu_frozen_bn.py and tests/test_frozen_bn_host.py).

Frozen BatchNorm = the reference modules under model.train() with every nn.BatchNorm2d in .eval(): the oracle's
`training=False` forward, whose float64 autograd over grad_check.oracle_leaves gives exactly the gradients of that regime.

`calibrated_sd` gives the seeded weights running statistics that are neither trivial (0 / 1) nor the test batch's own: one
train-mode oracle forward of a seeded calibration batch with momentum 1 (the running statistics become that batch's), then a
seeded perturbation  mean += 0.1 sqrt(var) n,  var *= U(0.7, 1.4).  A kernel that still normalised with batch statistics
would not pass against them (test_frozen_bn_host.py shows the size of the difference)."""
import contextlib

import torch
import torch.nn.functional as F

from conftest import rel_errors
from grad_check import canonical, model_grads, oracle_leaves
from train_step import build_model, forward_args

_CALIBRATED = {}  # variant -> state dict (the session's seed-0 weights of that variant: one calibration per variant)


@contextlib.contextmanager
def _momentum(value):
    from oracle import unet_oracle as U
    old = U.BN_MOMENTUM
    U.BN_MOMENTUM = value
    try:
        yield
    finally:
        U.BN_MOMENTUM = old


def _oracle_forward(variant, sd, x, t, cond, mag, training, stats=None):
    from oracle import unet_oracle as U
    if variant == "superres":
        return U.unet_forward(sd, x, t, cond, mag, training=training, stats=stats)
    if variant == "sar":
        return U.unet_forward_sar(sd, x, t, cond, training=training, stats=stats)
    if variant == "generation":
        return U.unet_forward_generation(sd, x, t, cond, training=training, stats=stats)
    raise ValueError(variant)


def calibration_batch(variant):
    """(x, t, cond, mag): a seeded batch of its own (B = 4, 32 x 32), not any test's."""
    from diffusionremotesensing_amd import synthetic
    t = torch.tensor([3, 400, 900, 1400])
    if variant == "superres":
        return (synthetic.tensor_normal("frozen.calib.x", (4, 3, 32, 32)), t,
                synthetic.tensor_uniform("frozen.calib.lr", (4, 3, 16, 16)), 2)
    if variant == "sar":
        return (synthetic.tensor_normal("frozen.calib.sar.x", (4, 1, 32, 32)), t,
                synthetic.tensor_uniform("frozen.calib.sar.sar", (4, 2, 32, 32)), 1)
    return synthetic.tensor_normal("frozen.calib.gen.x", (4, 3, 32, 32)), t, torch.tensor([1, 7, 7, 0]), 1


def calibrated_sd(variant, sd, seed=1234):
    """`sd` with calibrated, perturbed running statistics in every BatchNorm (both registered names of a ResConvBlock
    BatchNorm get the same tensor); float32 CPU tensors like `sd`.  Computed once per variant."""
    if variant in _CALIBRATED:
        return _CALIBRATED[variant]
    x, t, cond, mag = calibration_batch(variant)
    stats = {}
    with torch.no_grad(), _momentum(1.0):
        _oracle_forward(variant, sd, x, t, cond, mag, True, stats)
    gen = torch.Generator().manual_seed(seed)
    out = dict(sd)
    new = {}
    for pfx in sorted(stats):
        rm, rv = stats[pfx]
        rm = rm + 0.1 * rv.sqrt() * torch.randn(rm.shape, generator=gen)
        rv = rv * (0.7 + 0.7 * torch.rand(rv.shape, generator=gen))
        new[pfx] = (rm.float().contiguous(), rv.float().contiguous())
    seen = set()
    for k in sd:
        if k.endswith(".running_mean"):
            pfx = k[:-len(".running_mean")]
            rm, rv = new[canonical(pfx + ".")[:-1]]
            out[pfx + ".running_mean"], out[pfx + ".running_var"] = rm.clone(), rv.clone()
            seen.add(canonical(pfx + ".")[:-1])
    assert seen == set(new), sorted(seen ^ set(new))[:6]
    _CALIBRATED[variant] = out
    return out


def frozen_oracle_step(variant, sd, live, x, t, cond, noise, mag=1, dtype=torch.float64, training=False):
    """grad_check.oracle_step with the BatchNorm regime as an argument: (prediction, loss, {live name: gradient or None}).
    training=False is the frozen regime (running statistics of `sd`, which autograd treats as constants); training=True
    the batch-statistics regime on the same weights (the discrimination check)."""
    live = set(live)
    leaves = oracle_leaves(sd, {canonical(n) for n in live}, dtype)
    cond_d = cond.to(dtype) if (cond is not None and variant != "generation") else cond
    pred = _oracle_forward(variant, leaves, x.to(dtype), t, cond_d, mag, training, {} if training else None)
    loss = F.mse_loss(pred, noise.to(dtype))
    loss.backward()
    grads = {n: (None if leaves[n].grad is None else leaves[n].grad.detach().clone()) for n in live}
    return pred.detach(), loss.item(), grads


def bn_buffers(model):
    """{name: clone} of every running_mean / running_var / num_batches_tracked of the model."""
    return {k: b.detach().clone() for k, b in model.named_buffers()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def assert_bn_untouched(model, before):
    from guard import bits_equal
    after = bn_buffers(model)
    assert set(after) == set(before) and len(before) >= 3 * 20
    changed = [k for k in before if not bits_equal(before[k], after[k])]
    assert not changed, f"BatchNorm buffers written by a frozen step: {changed[:8]}"


def frozen_model(dev, variant, sd, train_impl=None, freeze=None):
    """A fresh train-mode model on `dev` with frozen BatchNorm (and the parameters `freeze(name)` selects frozen)."""
    m = build_model(dev, variant, sd)
    m.freeze_batchnorm()
    if train_impl is not None:
        m.hip_engine().set_impl(train_impl, train_impl=train_impl)
    if freeze is not None:
        for n, p in m.named_parameters():
            if freeze(n):
                p.requires_grad_(False)
    return m


def frozen_step(dev, variant, sd, x, t, cond, noise, mag=1, train_impl=None, freeze=None, oracle=None, put=lambda v, **kw: v):
    """The HIP frozen-BatchNorm step (forward, MSE, backward) against `oracle` = frozen_oracle_step(...) of the same batch
    with every parameter live.  Checks the prediction and the loss at train_step.step's forward bars (1e-4 for the exact-fp32
    plans, 1e-3 for the split-bf16 one) and that no BatchNorm buffer changed a bit; returns (HIP gradients, oracle gradients,
    prediction).  `put`: passes every device input through (guard.GuardedBlock.copy inside guarded allocations)."""
    m = frozen_model(dev, variant, sd, train_impl, freeze)
    assert m.training and not any(b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    before = bn_buffers(m)
    args = forward_args(dev, variant, x, t, cond, mag)
    args = tuple(put(a) if isinstance(a, torch.Tensor) else a for a in args)
    pred = m(*args)
    loss = F.mse_loss(pred, put(noise.to(dev)))
    loss.backward()
    torch.cuda.synchronize()
    m.hip_engine().check_faults()
    assert m.hip_engine()._last_plan.frozen
    got = model_grads(m)
    if oracle is None:
        oracle = frozen_oracle_step(variant, sd, list(got), x, t, cond, noise, mag)
    want, ref_loss, ref = oracle
    tol = 1e-3 if train_impl == "mfma_bf16x3" else 1e-4
    e_max, e_l2 = rel_errors(pred.detach().cpu(), want)
    print(f"  frozen prediction max-rel {e_max:.2e} rel-L2 {e_l2:.2e}; loss {loss.item():.6f} / {ref_loss:.6f}")
    assert e_l2 <= tol and e_max <= tol, ("prediction", e_max, e_l2)
    assert abs(loss.item() - ref_loss) <= tol * ref_loss, (loss.item(), ref_loss)
    assert_bn_untouched(m, before)
    return got, ref, pred.detach()
