"""CPU pins of the float64 gradient oracle and of the element-wise gradient check (tests/grad_check.py) that the GPU
gradient tests (tests/test_gpu_grads.py) rely on:
- the float64 oracle reproduces the reference's own fp32 gradient norms (G5, G8t, G9t) and the fp32 oracle tensor by
  tensor, so it is the same computation, only more exact;
- every indexing bug a weight-gradient or adjoint kernel can plausibly have fails the check by at least 5x its fp32-grade
  bar, including the ones that leave the gradient norm bit-identical.  Loosening the bar until it is blind fails here."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_inputs
from grad_check import MAX_REL_F32, REL_L2_F32, check_grads, grad_errors, grad_scale, oracle_step

HERE = os.path.dirname(os.path.abspath(__file__))


def _names(fname):
    return open(os.path.join(HERE, "golden", fname)).read().split()


def _g5(sd, dtype):
    from diffusionremotesensing_amd import synthetic
    x, t, lr = golden_inputs("g5", 4, 4, 3, 32, 2, 1500)
    noise = synthetic.tensor_normal("g5.noise", (4, 3, 32, 32))
    return oracle_step("superres", sd, _names("g5_param_names.txt"), x, t, lr, noise, 2, dtype)


@pytest.fixture(scope="module")
def g5_f64(seeded_sd):
    return _g5(seeded_sd, torch.float64)


@pytest.fixture(scope="module")
def g5_f32(seeded_sd):
    return _g5(seeded_sd, torch.float32)


def _assert_norms(grads, names, ref_norms, what):
    """Golden norms: < 0 marks a structurally unused parameter (no gradient).  Structural zeros (rounding noise in the
    reference) only have to stay small."""
    scale = float(ref_norms.max())
    bad = []
    for name, ref in zip(names, ref_norms):
        g = grads[name]
        if ref < 0:
            assert g is None, name
            continue
        got = g.norm().item()
        if ref < 1e-5 * scale:
            assert got < 1e-4 * scale, (name, got, float(ref))
        elif abs(got - ref) > 1e-4 * ref:
            bad.append((name, got, float(ref)))
    assert not bad, f"{what}: {bad[:8]}"


def test_fp32_oracle_path_is_unchanged(seeded_sd, golden):
    """The float64 support must not touch the fp32 oracle: its G5 training-step loss is the reference's to fp32 rounding."""
    _, loss, _, _ = _g5(seeded_sd, torch.float32)
    assert abs(loss - float(golden["g5_loss"])) <= 1e-6 * float(golden["g5_loss"])


def test_fp64_oracle_matches_g5_gradient_norms(g5_f64, golden):
    pred, loss, grads, _ = g5_f64
    assert pred.dtype == torch.float64
    assert abs(loss - float(golden["g5_loss"])) <= 1e-5 * float(golden["g5_loss"])
    _assert_norms(grads, _names("g5_param_names.txt"), golden["g5_grad_norms"], "g5")
    # the two full tensors the golden holds
    for key, name in (("g5_grad_output_bias", "output.bias"), ("g5_grad_conv0_weight", "conv0.weight")):
        ref = torch.from_numpy(golden[key]).double()
        assert ((grads[name] - ref).norm() / ref.norm()).item() < 1e-4, name


def test_fp64_oracle_matches_fp32_oracle_per_tensor(g5_f64, g5_f32):
    """fp32 ATen vs float64, tensor by tensor (1.2e-5 rel-L2 at most when written)."""
    _, _, g64, _ = g5_f64
    _, _, g32, _ = g5_f32
    _, _, worst = check_grads(g32, g64, 1e-3, what="fp32 oracle vs fp64 oracle (G5)")
    assert worst < 1e-4


def test_fp64_oracle_matches_variant_gradient_norms(seeded_sd_sar, seeded_sd_gen, vgolden):
    from diffusionremotesensing_amd import synthetic
    x = synthetic.tensor_normal("g8t.x", (4, 1, 32, 32))
    sar = synthetic.tensor_uniform("g8t.sar", (4, 2, 32, 32))
    noise = synthetic.tensor_normal("g8t.noise", (4, 1, 32, 32))
    names = _names("g8_param_names.txt")
    _, loss, grads, _ = oracle_step("sar", seeded_sd_sar, names, x, torch.from_numpy(vgolden["g8t_t"]), sar, noise)
    assert abs(loss - float(vgolden["g8t_loss"])) <= 1e-5 * float(vgolden["g8t_loss"])
    _assert_norms(grads, names, vgolden["g8t_grad_norms"], "g8t")

    x = synthetic.tensor_normal("g9t.x", (4, 3, 32, 32))
    noise = synthetic.tensor_normal("g9t.noise", (4, 3, 32, 32))
    names = _names("g9_param_names.txt")
    y = torch.from_numpy(vgolden["g9t_y"])
    _, loss, grads, _ = oracle_step("generation", seeded_sd_gen, names, x, torch.from_numpy(vgolden["g9t_t"]), y, noise)
    assert abs(loss - float(vgolden["g9t_loss"])) <= 1e-5 * float(vgolden["g9t_loss"])
    _assert_norms(grads, names, vgolden["g9t_grad_norms"], "g9t")
    ref = torch.from_numpy(vgolden["g9t_grad_label_emb"]).double()
    assert ((grads["label_emb.weight"] - ref).norm() / ref.norm()).item() < 1e-4


def _rot180(g):
    return g.flip(-1, -2)


def _transpose(g):
    assert g.shape[0] == g.shape[1]
    return g.transpose(0, 1).contiguous()


def _roll(g):
    return g.roll(1, dims=0)


def _negate_channel(g):
    g = g.clone()
    g[g.shape[0] // 2] = -g[g.shape[0] // 2]
    return g


def _scale(g):
    return g * 1.01


MUTATIONS = [
    ("taps rotated 180", "downs.1.weight", _rot180),
    ("taps rotated 180, 2x2", "attention_blocks.1.w_x.0.weight", _rot180),
    ("taps rotated 180, transposed conv", "ups.1.transform.weight", _rot180),
    ("ci-co transposed", "conv_blocks.2.conv2.0.weight", _transpose),
    ("ci-co transposed, 1x1", "attention_blocks.0.result.0.weight", _transpose),
    ("output channels rolled", "up_convs.1.weight", _roll),
    ("output channels rolled, bias", "bottle_neck.batch_norm2.bias", _roll),
    ("one output channel negated", "bottle_neck.conv2.0.weight", _negate_channel),
    ("scaled by 1.01", "output.weight", _scale),
    ("scaled by 1.01, deepest", "LR_encoder.blocks.0.conv1.weight", _scale),
]
SWAPS = [
    ("conv_blocks.1.batch_norm1.weight", "conv_blocks.1.batch_norm2.weight"),
    ("attention_blocks.0.w_g.0.weight", "attention_blocks.0.result.0.weight"),
    ("bottle_neck.conv2.0.weight", "ups.0.conv.weight"),
]


@pytest.mark.parametrize("what,name,fn", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_check_fails_on_mutation(g5_f64, what, name, fn):
    _, _, grads, _ = g5_f64
    check_grads(grads, grads, 0.0, 0.0, "unmutated")  # the reference passes itself exactly
    got = dict(grads)
    got[name] = fn(grads[name])
    assert not torch.equal(got[name], grads[name]), what
    errs, hard = grad_errors(got, grads)
    assert not hard
    e_max, e_l2 = errs[name]
    print(f"{what} on {name}: max-rel {e_max:.2e} rel-L2 {e_l2:.2e} "
          f"(norm change {abs(got[name].norm() / grads[name].norm() - 1).item():.1e})")
    assert e_l2 >= 5 * REL_L2_F32, (what, e_max, e_l2)
    with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
        check_grads(got, grads, REL_L2_F32, MAX_REL_F32, what)


@pytest.mark.parametrize("a,b", SWAPS, ids=["bn1-bn2", "w_g-result", "bottleneck-conv2-ups0-conv"])
def test_check_fails_on_swapped_gradients(g5_f64, a, b):
    _, _, grads, _ = g5_f64
    assert grads[a].shape == grads[b].shape
    got = dict(grads)
    got[a], got[b] = grads[b], grads[a]
    errs, _ = grad_errors(got, grads)
    assert min(errs[a][1], errs[b][1]) >= 5 * REL_L2_F32, (errs[a], errs[b])
    with pytest.raises(AssertionError):
        check_grads(got, grads, REL_L2_F32, MAX_REL_F32, "swapped")


def test_check_rules_for_unused_and_structural_zeros(g5_f64):
    _, _, grads, _ = g5_f64
    unused = [n for n, g in grads.items() if g is None]
    assert unused, "the superres trunk has structurally unused parameters (conv_upsampled_lr_img of blocks 1..3)"
    scale = max(g.norm().item() for g in grads.values() if g is not None)
    zeros = [n for n, g in grads.items() if g is not None and g.norm().item() < 1e-5 * scale]
    assert zeros, "conv biases in front of a BatchNorm have a zero true gradient"
    got = dict(grads)
    got[unused[0]] = torch.zeros(1)
    with pytest.raises(AssertionError, match="unused"):
        check_grads(got, grads, REL_L2_F32, MAX_REL_F32)
    got = dict(grads)
    got["conv0.weight"] = None
    with pytest.raises(AssertionError, match="no gradient"):
        check_grads(got, grads, REL_L2_F32, MAX_REL_F32)
    got = dict(grads)
    got[zeros[0]] = torch.full_like(grads[zeros[0]], 1e-3 * scale)
    with pytest.raises(AssertionError, match="structural zero"):
        check_grads(got, grads, REL_L2_F32, MAX_REL_F32)
    got = dict(grads)  # rounding noise on a structural zero is fine
    got[zeros[0]] = torch.full_like(grads[zeros[0]], 1e-7 * scale)
    check_grads(got, grads, REL_L2_F32, MAX_REL_F32)


# ---- what the frozen-slot tests (tests/test_gpu_backward_contract.py) rely on ------------------------------------------
def test_check_fails_on_wanted_gradient_left_at_zero(g5_f64):
    """A backward that skips a wanted slot leaves the zeros of its clearing pass: that fails, for a large tensor and for the
    smallest live one alike."""
    _, _, grads, _ = g5_f64
    errs, _ = grad_errors(grads, grads)
    smallest = min(errs, key=lambda n: grads[n].norm().item())
    for name in ("bottle_neck.time_mlp.2.weight", "conv_blocks.1.time_mlp.0.bias", smallest):
        got = dict(grads)
        got[name] = torch.zeros_like(grads[name])
        e, hard = grad_errors(got, grads)
        assert not hard and abs(e[name][1] - 1.0) < 1e-12, (name, e[name])
        with pytest.raises(AssertionError, match=name.replace(".", r"\.")):
            check_grads(got, grads, REL_L2_F32, MAX_REL_F32, "zeros")


def test_check_fails_on_label_gradient_without_one_mlp(seeded_sd_gen):
    """d(label_emb.weight) is the sum of one share per time MLP (every MLP reads e = posenc(t) + label_emb[y]).  The shares
    come from the oracle itself: with an MLP's first bias given per sample, its gradient is d(pre1) per sample, and the
    share is that times W1, added onto the rows of the samples' classes.  Dropping any one share fails the check."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    names = [n for n, _ in Residual_Attention_UNet_generation(3, 3, 10, "cpu").named_parameters()]
    x = synthetic.tensor_normal("grads.gen.x", (3, 3, 24, 40))
    noise = synthetic.tensor_normal("grads.gen.noise", (3, 3, 24, 40))
    t, y = torch.tensor([1, 800, 1499]), torch.tensor([4, 9, 4])
    b1s = [n for n in names if n.endswith(".time_mlp.0.bias")]
    assert len(b1s) == 7
    sd = dict(seeded_sd_gen)
    for n in b1s:
        sd[n] = sd[n].expand(3, -1).clone()  # F.linear broadcasts it: same forward, one gradient row per sample
    _, loss, grads, _ = oracle_step("generation", sd, names, x, t, y, noise)
    _, loss0, grads0, _ = oracle_step("generation", seeded_sd_gen, names, x, t, y, noise)
    assert loss == loss0
    full = grads0["label_emb.weight"]
    assert torch.equal(grads["label_emb.weight"], full)
    shares = {}
    for n in b1s:
        w1 = seeded_sd_gen[n[:-len("bias")] + "weight"].double()
        shares[n] = torch.zeros_like(full).index_add_(0, y, grads[n] @ w1)
        assert ((grads[n].sum(0) - grads0[n]).norm() / grads0[n].norm()).item() < 1e-12
    assert ((sum(shares.values()) - full).norm() / full.norm()).item() < 1e-12
    for n, share in shares.items():
        got = dict(grads0)
        got["label_emb.weight"] = full - share
        errs, hard = grad_errors(got, grads0)
        e_max, e_l2 = errs["label_emb.weight"]
        print(f"label gradient without the share of {n[:-len('.time_mlp.0.bias')]}: max-rel {e_max:.2e} rel-L2 {e_l2:.2e}")
        assert not hard and e_l2 >= 5 * REL_L2_F32, (n, e_max, e_l2)
        with pytest.raises(AssertionError, match=r"label_emb\.weight"):
            check_grads(got, grads0, REL_L2_F32, MAX_REL_F32, "label share")


def test_subset_with_full_scale_keeps_the_structural_zeros(g5_f64):
    """With some parameters frozen only a subset is compared.  Its structural zeros are those of the full set when the
    full set's scale is handed in; measured against the subset's own largest gradient they would not be."""
    _, _, grads, _ = g5_f64
    scale = grad_scale(grads)
    full_errs, hard = grad_errors(grads, grads)
    assert not hard
    zeros = {n for n, g in grads.items() if g is not None and n not in full_errs}
    assert len(zeros) >= 8
    live = sorted(full_errs, key=lambda n: grads[n].norm().item())
    # (a) the zeros and the three smallest live tensors; (b) the zeros alone; (c) every seventh name
    for subset in (zeros | set(live[:3]), zeros, set(list(grads)[::7])):
        sub = {n: grads[n] for n in subset}
        errs, hard = grad_errors(sub, sub, scale)
        assert not hard and set(errs) == set(full_errs) & subset, sorted(set(errs) ^ (set(full_errs) & subset))
        noisy = {n: (g + 1e-3 * scale if n in zeros else g) for n, g in sub.items() if g is not None}
        noisy.update({n: None for n, g in sub.items() if g is None})
        _, hard = grad_errors(noisy, sub, scale)
        assert {h[0] for h in hard} == zeros & subset
    # without the full scale the largest structural zero of (b) would be held to the relative bars as if it were live
    own, _ = grad_errors({n: grads[n] for n in zeros}, {n: grads[n] for n in zeros})
    assert own, "the subset's own scale turns a structural zero into a live tensor"
