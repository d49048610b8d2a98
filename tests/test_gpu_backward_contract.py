"""The UNet backward outside the one configuration the other gradient tests run it in (every parameter live, a dense MSE
dout, one forward then one backward).  include/drs_hip.h promises more, and so does engine.py:

- NULL gradient slots: `grads[i]` may be NULL ("skip"), which is what HipUNetEngine.backward passes for a parameter with
  requires_grad False.  Each frozen set below steers the launchers into the branches that serve such slots (the bare column
  sum of wgrad() when only the bias is wanted, the slice layout of the MFMA weight-gradient kernels without a bias row, the
  scratch sinks of the BatchNorm / psi backward, the per-pointer stores of the time-MLP kernel, bwd_zero_grads over ranges
  with holes) and compares every WANTED gradient element-wise with the float64 oracle (tests/grad_check.py); the frozen ones
  must come back as None.  The oracle step is computed once per variant with every parameter live: freezing a parameter
  does not change any other parameter's gradient.  A structural zero stays one: the threshold is the full set's (scale=).
- other upstream gradients: impulses at the four image corners (the border handling of every data-gradient kernel), ones
  delivered as the expanded stride-0 tensor of pred.sum().backward(), one image with a zero gradient, a permuted
  (non-contiguous) dout.
- accumulation of two micro-batches of different shape into one .grad (the first .grad aliases the first flat buffer).
- pairing: the backward reads the plan's workspace as its own forward left it and consumes it, so a backward whose
  forward is no longer the plan's last one, or that runs a second time, raises before anything is launched.

Bars: grad_check.REL_L2_F32 / MAX_REL_F32 (rel-L2 <= 1e-3, max-rel <= 5e-3 on every tensor), on the training default plan
(and `direct` where a case says so).  The CPU oracle in fp32 against fp64 on the superres batch: worst rel-L2 4.5e-5 (MSE),
3.0e-6 (corners), 2.7e-5 (ones), 4.5e-6 (one-image), the same 27 structural zeros in each.

Measured on MI355X (worst tensor by rel-L2 of each case):
  frozen sets, superres: weights-frozen 6.2e-5 (attention_blocks.0.psi.0.bias) / direct 4.1e-6; biases-and-norms-frozen 1.9e-5
  (LR_encoder.blocks.0.conv1.weight) / direct 4.6e-6; mlp-second-linear-only 1.8e-5, mlp-first-linear-only 1.6e-5, mlp-mixed
  6.2e-5, decoder-only 6.2e-5, every-seventh 2.0e-5; generation label-emb-only 6.1e-6, label-emb-frozen 6.8e-4
  (attention_blocks.0.psi.0.bias, the cancelling sum test_gpu_grads.py describes); SAR weights-frozen 1.3e-4.
  dout: corners 6.6e-5, ones 2.8e-5, one-image 1.4e-4 (attention_blocks.1.psi.0.bias), permuted 5.1e-5.
  two micro-batches 3.3e-5 with either cache size, running statistics after both steps 2.8e-7; a fresh step after a refused
  backward 6.2e-5, the same figure as the `tiny` case of test_gpu_grads.py.
"""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from grad_check import MAX_REL_F32, REL_L2_F32, check_grads, grad_scale, model_grads, oracle_step
from guard import bits_equal, guarded_allocations
from train_step import build_model, check_running_stats, forward_args, step

pytestmark = pytest.mark.gpu

T_MAX = 1499


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


# ---- batches and their oracle steps (computed once, shared, never modified) ---------------------------------------------
_TREES = {}


def _tree(variant):
    """(parameter names in named_parameters() order, names of every conv / linear / ConvTranspose weight) of a variant."""
    if variant not in _TREES:
        m = _cpu_model(variant)
        names = [n for n, _ in m.named_parameters()]
        kinds = (nn.Conv2d, nn.Linear, nn.ConvTranspose2d)
        weights = {f"{k}.weight" for k, mod in m.named_modules() if isinstance(mod, kinds)} & set(names)
        _TREES[variant] = (names, weights)
    return _TREES[variant]


def _cpu_model(variant):
    if variant == "superres":
        from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
        return Residual_Attention_UNet_superres(3, 3, "cpu")
    if variant == "sar":
        from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
        return Residual_Attention_UNet_SAR_TO_NDVI(2, 1, "cpu")
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    return Residual_Attention_UNet_generation(3, 3, 10, "cpu")


def _superres_batch():
    """test_gpu_grads' `tiny` case: B=2, 24x40, x2 (3x5 bottleneck, partial tiles at every level), timesteps 1 and T-1."""
    from diffusionremotesensing_amd import synthetic
    return (synthetic.tensor_normal("grads.tiny.x", (2, 3, 24, 40)), torch.tensor([1, T_MAX]),
            synthetic.tensor_uniform("grads.tiny.lr", (2, 3, 12, 20)), synthetic.tensor_normal("grads.tiny.noise", (2, 3, 24, 40)), 2)


def _small_batch():
    """The second micro-batch: B=1, 32x32, x2."""
    from diffusionremotesensing_amd import synthetic
    return (synthetic.tensor_normal("contract.small.x", (1, 3, 32, 32)), torch.tensor([700]),
            synthetic.tensor_uniform("contract.small.lr", (1, 3, 16, 16)), synthetic.tensor_normal("contract.small.noise", (1, 3, 32, 32)), 2)


@pytest.fixture(scope="module")
def sr(seeded_sd):
    """(batch, oracle step) of the superres case."""
    batch = _superres_batch()
    return batch, oracle_step("superres", seeded_sd, _tree("superres")[0], *batch)


@pytest.fixture(scope="module")
def small(seeded_sd, sr):
    """(batch, oracle step) of the second micro-batch, the oracle chained: it starts from the running statistics the first
    step left (float64), so its statistics are those after both steps.  The gradients do not depend on them."""
    sd = dict(seeded_sd)
    for k, (rm, rv) in sr[1][3].items():
        sd[k + ".running_mean"], sd[k + ".running_var"] = rm, rv
    batch = _small_batch()
    return batch, oracle_step("superres", sd, _tree("superres")[0], *batch)


@pytest.fixture(scope="module")
def gen(seeded_sd_gen):
    from diffusionremotesensing_amd import synthetic
    batch = (synthetic.tensor_normal("grads.gen.x", (3, 3, 24, 40)), torch.tensor([1, 800, T_MAX]), torch.tensor([4, 9, 4]),
             synthetic.tensor_normal("grads.gen.noise", (3, 3, 24, 40)), 1)
    return batch, oracle_step("generation", seeded_sd_gen, _tree("generation")[0], *batch)


@pytest.fixture(scope="module")
def sar(seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    batch = (synthetic.tensor_normal("grads.sar.x", (2, 1, 40, 24)), torch.tensor([T_MAX, 1]),
             synthetic.tensor_uniform("grads.sar.sar", (2, 2, 40, 24)), synthetic.tensor_normal("grads.sar.noise", (2, 1, 40, 24)), 1)
    return batch, oracle_step("sar", seeded_sd_sar, _tree("sar")[0], *batch)


# ---- frozen sets ----------------------------------------------------------------------------------------------------------
DECODER = ("ups.", "up_convs.", "attention_blocks.", "gating_signals.", "output.")


def _mlp_prefixes(variant):
    """The time MLPs in module order ("conv_blocks.0.time_mlp", ..., "ups.2.time_mlp")."""
    out = []
    for n in _tree(variant)[0]:
        if n.endswith(".time_mlp.0.weight"):
            out.append(n[:-len(".0.weight")])
    assert len(out) == 7, out
    return out


def _freeze(variant, case):
    """Predicate on parameter names: True = frozen."""
    names, weights = _tree(variant)
    if case == "weights-frozen":
        return lambda n: n in weights
    if case == "biases-and-norms-frozen":
        return lambda n: n not in weights
    if case == "mlp-second-linear-only":
        return lambda n: ".time_mlp.2." not in n
    if case == "mlp-first-linear-only":
        return lambda n: ".time_mlp.0." not in n
    if case == "mlp-mixed":
        mlps = _mlp_prefixes(variant)
        whole = tuple(p + "." for p in mlps[0::2])
        first_w = {p + ".0.weight" for p in mlps[1::2]}
        return lambda n: n.startswith(whole) or n in first_w
    if case == "decoder-only":
        return lambda n: not n.startswith(DECODER)
    if case == "every-seventh":
        keep = set(names[::7])
        return lambda n: n not in keep
    if case == "label-emb-only":
        return lambda n: n != "label_emb.weight"
    if case == "label-emb-frozen":
        return lambda n: n == "label_emb.weight"
    raise ValueError(case)


def _frozen_step(dev, variant, sd, fixture, case, impl):
    batch, oracle = fixture
    freeze = _freeze(variant, case)
    names = _tree(variant)[0]
    frozen = [n for n in names if freeze(n)]
    wanted = [n for n in names if not freeze(n)]
    assert frozen and wanted and any(oracle[2][n] is not None for n in wanted), (len(frozen), len(wanted))
    # (step: prediction, loss, every BatchNorm's running statistics, check_faults)
    got, ref = step(dev, variant, sd, *batch, train_impl=impl, freeze=freeze, oracle=oracle)
    assert list(got) == names
    leaked = [n for n in frozen if got[n] is not None]
    assert not leaked, f"frozen parameters with a gradient: {leaked[:8]}"
    check_grads({n: got[n] for n in wanted}, {n: ref[n] for n in wanted}, REL_L2_F32, MAX_REL_F32,
                f"{variant} {case} [{impl or 'default'}] ({len(wanted)} wanted, {len(frozen)} frozen)", scale=grad_scale(ref))


SUPERRES_FROZEN = [("weights-frozen", None), ("weights-frozen", "direct"), ("biases-and-norms-frozen", None),
                   ("biases-and-norms-frozen", "direct"), ("mlp-second-linear-only", None), ("mlp-first-linear-only", None),
                   ("mlp-mixed", None), ("decoder-only", None), ("every-seventh", None)]


@pytest.mark.parametrize("case,impl", SUPERRES_FROZEN, ids=[f"{c}-{i or 'default'}" for c, i in SUPERRES_FROZEN])
def test_frozen_superres(dev, seeded_sd, sr, case, impl):
    _frozen_step(dev, "superres", seeded_sd, sr, case, impl)


@pytest.mark.parametrize("case", ["label-emb-only", "label-emb-frozen"])
def test_frozen_generation(dev, seeded_sd_gen, gen, case):
    """label-emb-only: no MLP slot is wanted, yet every MLP's share of d(label_emb.weight) is; label-emb-frozen: dlabel NULL."""
    _frozen_step(dev, "generation", seeded_sd_gen, gen, case, None)


def test_frozen_sar_weights(dev, seeded_sd_sar, sar):
    """The 2-band stem and the 1-channel head with only their biases wanted."""
    _frozen_step(dev, "sar", seeded_sd_sar, sar, "weights-frozen", None)


def test_freeze_sets_are_what_they_claim():
    """The name sets behind the cases (no device needed beyond the module's mark): complements, MLP slots, holes."""
    names, weights = _tree("superres")
    assert {"conv0.weight", "ups.1.transform.weight", "bottle_neck.time_mlp.2.weight", "output.weight"} <= weights
    assert not any("batch_norm" in n or n.endswith(".bias") for n in weights) and "attention_blocks.0.result.1.weight" not in weights
    assert "label_emb.weight" not in _tree("generation")[1]
    f, g = _freeze("superres", "weights-frozen"), _freeze("superres", "biases-and-norms-frozen")
    assert all(f(n) != g(n) for n in names)
    mixed = _freeze("superres", "mlp-mixed")
    assert [n for n in names if "time_mlp" not in n and mixed(n)] == []
    assert all(mixed(f"conv_blocks.0.time_mlp.{s}") for s in ("0.weight", "0.bias", "2.weight", "2.bias"))
    assert [mixed(f"conv_blocks.1.time_mlp.{s}") for s in ("0.weight", "0.bias", "2.weight", "2.bias")] == [True, False, False, False]
    assert sum(not _freeze("superres", "every-seventh")(n) for n in names) == len(names[::7])


# ---- upstream gradients -----------------------------------------------------------------------------------------------
class _Loss:
    """A scalar of the prediction whose backward delivers `dense` (as the oracle gets it) in some other layout."""

    def __init__(self, fn, dense):
        self.fn, self.dense = fn, dense

    def __call__(self, pred):
        return self.fn(pred)


def _douts():
    from diffusionremotesensing_amd import synthetic
    shape = (2, 3, 24, 40)
    corners = torch.zeros(shape)
    corners[0, 0, 0, 0], corners[0, 1, 0, 39], corners[1, 2, 23, 0], corners[1, 0, 23, 39] = 1.0, -0.7, 0.5, -1.3
    one_image = synthetic.tensor_normal("contract.dout.one-image", shape).clone()
    one_image[0] = 0.0
    w = synthetic.tensor_normal("contract.dout.permuted", (2, 3, 40, 24))
    return {
        "corners": corners,
        "ones": _Loss(lambda pred: pred.sum(), torch.ones(shape)),
        "one-image": one_image,
        "permuted": _Loss(lambda pred: (pred.permute(0, 1, 3, 2) * w.to(pred.device)).sum(), w.permute(0, 1, 3, 2).contiguous()),
    }


@pytest.mark.parametrize("which", ["corners", "ones", "one-image", "permuted"])
def test_upstream_gradient(monkeypatch, dev, seeded_sd, which):
    from diffusionremotesensing_amd.engine import HipUNetEngine
    dout = _douts()[which]
    seen = []
    real = HipUNetEngine.backward

    def backward(self, plan, x, timestep, d, labels=None):
        seen.append((tuple(d.shape), tuple(d.stride()), d.is_contiguous()))
        return real(self, plan, x, timestep, d, labels)
    monkeypatch.setattr(HipUNetEngine, "backward", backward)
    got, ref = step(dev, "superres", seeded_sd, *_superres_batch(), dout=dout)
    assert len(seen) == 1 and seen[0][0] == (2, 3, 24, 40)
    if which == "ones":
        assert seen[0][1] == (0, 0, 0, 0), f"the engine was to receive the expanded tensor, got strides {seen[0][1]}"
    elif which == "permuted":
        assert not seen[0][2] and seen[0][1] == (2880, 960, 1, 24), f"the engine was to receive a permuted view, got strides {seen[0][1]}"
    check_grads(got, ref, REL_L2_F32, MAX_REL_F32, f"dout {which}")


# ---- accumulation -------------------------------------------------------------------------------------------------------
def _sum(a, b):
    return b if a is None else a if b is None else a + b


@pytest.mark.parametrize("max_plans", [None, 1], ids=["default-cache", "max-plans-1"])
def test_two_micro_batches_accumulate(dev, seeded_sd, sr, small, max_plans):
    """B=2 24x40, then B=1 32x32, into one .grad without zero_grad: the sum of the two oracle gradients; with max_plans = 1
    the first plan has left the cache when the second one is built."""
    m = build_model(dev, "superres", seeded_sd)
    eng = m.hip_engine()
    if max_plans is not None:
        eng.max_plans = max_plans
    for (x, t, lr, noise, mag), _ in (sr, small):
        pred = m(*forward_args(dev, "superres", x, t, lr, mag))
        F.mse_loss(pred, noise.to(dev)).backward()
    torch.cuda.synchronize()
    eng.check_faults()
    if max_plans is not None:
        assert len(eng._plans) == 1
    got = model_grads(m)
    ref = {n: _sum(sr[1][2][n], small[1][2][n]) for n in got}
    check_grads(got, ref, REL_L2_F32, MAX_REL_F32, f"two micro-batches [{max_plans or 'default'} plans]")
    worst = check_running_stats(m.state_dict(), small[1][3], seeded_sd, 1e-4, steps=2)
    print(f"  running statistics after two steps: worst {worst[0]:.2e} ({worst[1]})")


# ---- pairing of forward and backward ------------------------------------------------------------------------------------
def _grads_bits(m):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m.named_parameters()}


def _valid_step(m, args, noise):
    pred = m(*args)
    loss = F.mse_loss(pred, noise)
    return pred, loss


@pytest.mark.parametrize("case", ["backward-of-the-earlier-forward", "second-backward", "no-grad-forward-between"])
def test_unpaired_backward_raises_before_any_launch(monkeypatch, dev, seeded_sd, sr, case):
    """Inside guarded allocations (tests/guard.py): the raise comes before any drs_* call and any allocation, the .grad
    buffers of the step before keep their bits, no guard is damaged; then a fresh forward + backward is right."""
    (x, t, lr, noise, mag), oracle = sr
    with guarded_allocations(monkeypatch, dev, "aligned") as block:
        m = build_model(dev, "superres", seeded_sd)
        eng = m.hip_engine()
        args, noise_d = forward_args(dev, "superres", x, t, lr, mag), noise.to(dev)
        if case == "second-backward":
            _, loss = _valid_step(m, args, noise_d)
            loss.backward(retain_graph=True)
            match = "ran twice"
        else:
            _valid_step(m, args, noise_d)[1].backward()  # a step before: .grad holds its gradients (views of a guarded flat buffer)
            _, loss = _valid_step(m, args, noise_d)
            if case == "backward-of-the-earlier-forward":
                _valid_step(m, args, noise_d)
            else:
                with torch.no_grad():
                    m(*args)
            match = "later train-mode forward"
        torch.cuda.synchronize()
        before = _grads_bits(m)
        assert sum(g is not None for g in before.values()) > 100
        block.calls.clear()
        n_alloc = len(block.allocations)
        with pytest.raises(RuntimeError, match=match):
            loss.backward()
        torch.cuda.synchronize()
        assert not block.calls, f"the library was called before the raise: {sorted(block.calls)}"
        assert len(block.allocations) == n_alloc, "a buffer was allocated before the raise"
        after = _grads_bits(m)
        changed = [n for n in before if not bits_equal(before[n], after[n])]
        assert not changed, f".grad changed by a backward that raised: {changed[:8]}"
        # a fresh pair is correct
        m.zero_grad(set_to_none=True)
        _valid_step(m, args, noise_d)[1].backward()
        torch.cuda.synchronize()
        eng.check_faults()
        check_grads(model_grads(m), oracle[2], REL_L2_F32, MAX_REL_F32, f"fresh step after {case}")


def test_forward_of_another_shape_between_is_fine(dev, seeded_sd, sr, small):
    """Another shape runs on another plan: the first forward's workspace is untouched and its backward is right.  The
    second shape's own node is stale by then (its plan saw the no_grad forward) and says so."""
    m = build_model(dev, "superres", seeded_sd)
    (x, t, lr, noise, mag), oracle = sr
    (x2, t2, lr2, noise2, mag2), oracle2 = small
    loss1 = F.mse_loss(m(*forward_args(dev, "superres", x, t, lr, mag)), noise.to(dev))
    loss2 = F.mse_loss(m(*forward_args(dev, "superres", x2, t2, lr2, mag2)), noise2.to(dev))
    with torch.no_grad():  # and one outside autograd
        m(*forward_args(dev, "superres", x2, t2, lr2, mag2))
    loss1.backward()
    torch.cuda.synchronize()
    m.hip_engine().check_faults()
    check_grads(model_grads(m), oracle[2], REL_L2_F32, MAX_REL_F32, "backward after a forward of another shape")
    with pytest.raises(RuntimeError, match="later train-mode forward"):
        loss2.backward()  # (its own plan did see a later forward: the no_grad one)
