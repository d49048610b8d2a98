"""Element-wise gradient check of a training step against the float64 oracle (a plain module, imported by the tests).

`oracle_step` runs one training step (train-mode forward, MSE against the given noise, autograd backward) of the CPU
oracle in float64 and returns every parameter's gradient; `check_grads` compares a HIP model's gradients with them
tensor by tensor (max-rel and rel-L2 of conftest.rel_errors).  A gradient norm cannot see an index bug: rotated taps, a
transposed square dW, permuted channels or two swapped same-shape gradients all keep it; tests/test_grad_check_selftest.py
shows that each of them fails this check."""
import torch
import torch.nn.functional as F

from conftest import rel_errors

# fp32-grade bars (training default, mfma_f32 and direct train plans) and the opt-in split-bf16 training bar
REL_L2_F32, MAX_REL_F32 = 1e-3, 5e-3
REL_L2_BF16X3 = 5e-2
# a true gradient below this fraction of the largest one is structurally zero (a conv bias in front of a BatchNorm):
# both sides hold rounding noise there, and the gradient only has to be small
ZERO_FRAC, ZERO_TOL = 1e-5, 1e-4

# the modules register every ResConvBlock BatchNorm twice (Sequential slot and named attribute): one leaf for both names
BN_ALIASES = ((".conv1.1.", ".batch_norm1."), (".conv2.1.", ".batch_norm2."), (".shortcut_conv.1.", ".shortcut_batch_norm."))


def canonical(name):
    for a, b in BN_ALIASES:
        name = name.replace(a, b)
    return name


def oracle_leaves(sd, live, dtype=torch.float64):
    """The state_dict in `dtype`, with the parameters named in `live` as leaves that require a gradient."""
    out = {}
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            v = v.detach().to(dtype).clone()
            if k in live and canonical(k) == k:
                v.requires_grad_(True)
        else:
            v = v.clone()
        out[k] = v
    for k in out:
        out[k] = out[canonical(k)]
    return out


def oracle_step(variant, sd, live, x, t, cond, noise, mag=1, dtype=torch.float64, dout=None):
    """One training step of the oracle: (prediction, loss, {live name: gradient or None}, {BatchNorm prefix: (running_mean,
    running_var)}).  `cond` is the LR image (superres), the SAR image (sar) or the labels (generation; None = unconditional).
    With `dout` (a tensor of the prediction's shape) the backward is pred.backward(dout) instead of the MSE's: `noise` is
    not read and the loss returned is sum(pred * dout), the scalar that has this upstream gradient."""
    from oracle import unet_oracle as U
    live = set(live)
    leaves = oracle_leaves(sd, {canonical(n) for n in live}, dtype)
    x = x.to(dtype)
    stats = {}
    if variant == "superres":
        pred = U.unet_forward(leaves, x, t, cond.to(dtype), mag, training=True, stats=stats)
    elif variant == "sar":
        pred = U.unet_forward_sar(leaves, x, t, cond.to(dtype), training=True, stats=stats)
    elif variant == "generation":
        pred = U.unet_forward_generation(leaves, x, t, cond, training=True, stats=stats)
    else:
        raise ValueError(variant)
    if dout is None:
        loss = F.mse_loss(pred, noise.to(dtype))
        loss.backward()
    else:
        dout = dout.to(dtype)
        loss = (pred.detach() * dout).sum()
        pred.backward(dout)
    grads = {n: (None if leaves[n].grad is None else leaves[n].grad.detach().clone()) for n in live}
    stats = {k: (rm.detach(), rv.detach()) for k, (rm, rv) in stats.items()}
    return pred.detach(), loss.item(), grads, stats


def model_grads(model):
    """{parameter name: gradient on the host, or None} of a model after loss.backward()."""
    return {n: (None if p.grad is None else p.grad.detach().cpu()) for n, p in model.named_parameters()}


def grad_scale(ref):
    """The norm of the largest true gradient: what a structural zero is measured against."""
    return max(r.norm().item() for r in ref.values() if r is not None)


def grad_errors(got, ref, scale=None):
    """{name: (max-rel, rel-L2)} of every parameter with a live, non-negligible true gradient, and the list of problems
    that no tolerance excuses (a missing or extra gradient, the wrong shape, a structural zero that is not small).
    `scale`: grad_scale of the FULL gradient set when `ref` is a subset of it (some parameters frozen), so that the same
    tensors count as structural zeros as in the full comparison; default: grad_scale(ref)."""
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref)))[:8]
    if scale is None:
        scale = grad_scale(ref)
    errs, hard = {}, []
    for name, r in ref.items():
        g = got[name]
        if r is None:
            if g is not None:
                hard.append((name, "unused parameter got a gradient"))
            continue
        if g is None:
            hard.append((name, "no gradient"))
            continue
        if tuple(g.shape) != tuple(r.shape):
            hard.append((name, f"shape {tuple(g.shape)} != {tuple(r.shape)}"))
            continue
        if r.norm().item() < ZERO_FRAC * scale:
            if not g.double().norm().item() < ZERO_TOL * scale:
                hard.append((name, f"structural zero has norm {g.double().norm().item():.3e}"))
            continue
        errs[name] = rel_errors(g, r)
    return errs, hard


def check_grads(got, ref, rel_l2, max_rel=None, what="", scale=None):
    """Assert every gradient of `got` against `ref` (see grad_errors); returns (worst name, max-rel, rel-L2) by rel-L2 and
    prints it."""
    errs, hard = grad_errors(got, ref, scale)
    bad = [(n, e_max, e_l2) for n, (e_max, e_l2) in errs.items()
           if not (e_l2 <= rel_l2 and (max_rel is None or e_max <= max_rel))]
    worst = max(errs.items(), key=lambda kv: kv[1][1])
    worst_max = max(errs.items(), key=lambda kv: kv[1][0])
    print(f"{what}: {len(errs)} tensors; worst rel-L2 {worst[1][1]:.2e} ({worst[0]}), "
          f"worst max-rel {worst_max[1][0]:.2e} ({worst_max[0]})")
    bad.sort(key=lambda b: -b[2])
    assert not hard and not bad, f"{what}: {hard[:6]} " + ", ".join(f"{n}: max-rel {a:.2e} rel-L2 {b:.2e}" for n, a, b in bad[:8])
    return worst[0], worst[1][0], worst[1][1]
