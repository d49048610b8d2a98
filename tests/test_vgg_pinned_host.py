"""The pinned float64 references of tests/vgg_pinned.py, on the CPU: they restate the same function as autograd, an exact
fp32 run sits four orders of magnitude closer to them than to the free float64 oracle, and a single broken step of the
backward moves d(loss)/d(pred) far beyond the bar tests/test_gpu_perceptual_layers.py holds the device to.

torch fp32 on the CPU stands in for the device.  The mutation table (MUTATIONS) records, per mutation and shape, the effect
measured here as (max-rel, rel-L2) of conftest.rel_errors between the mutated and the exact pinned backward.
"""
import pytest
import torch
import torch.nn.functional as F

import vgg_oracle as O
import vgg_pinned as P
from conftest import rel_errors

# (B, H, W, near): the cases of tests/test_gpu_perceptual_layers.py
CASES = [(1, 40, 224, False), (3, 72, 224, False), (1, 224, 224, False), (1, 24, 40, False), (1, 300, 260, False),
         (2, 40, 224, True)]
IDS = [f"B{c[0]}_{c[1]}x{c[2]}{'_near' if c[3] else ''}" for c in CASES]
GPU_BAR_CEILING = 1e-3  # the device's dpred bar may not exceed this (test_gpu_perceptual_layers.DPRED_BAR_CEILING)
GRAD_LOSS = 0.7
_RUNS = {}


@pytest.fixture(scope="module")
def vgg_sd():
    return O.seeded_vgg_state_dict()


def pair(B, H, W, near):
    from diffusionremotesensing_amd import synthetic
    x = synthetic.tensor_normal(f"vggl.x.{B}.{H}.{W}", (B, 3, H, W))
    if near:
        return x, x + 0.05 * synthetic.tensor_normal(f"vggl.n.{B}.{H}.{W}", (B, 3, H, W))
    return x, synthetic.tensor_normal(f"vggl.y.{B}.{H}.{W}", (B, 3, H, W))


def _fp32_run(sd, case):
    """torch fp32 run of a case and the exact pinned backward of its activations, computed once."""
    if case not in _RUNS:
        x0, saved, feats, loss, dpred = P.run_torch(sd, *pair(*case), torch.float32, GRAD_LOSS)
        want = P.pinned_backward(sd, saved, feats, GRAD_LOSS, case[1:3])
        _RUNS[case] = dict(saved=saved, feats=feats, dpred=dpred, want=want)
    return _RUNS[case]


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_pinned_backward_is_the_autograd_backward_in_float64(vgg_sd, case):
    """Fed float64 activations, pinned_backward equals float64 autograd of vgg_oracle.vgg_loss: the same function."""
    x, y = pair(*case)
    _, saved, feats, loss, _ = P.run_torch(vgg_sd, x, y, torch.float64)
    want_loss, want = O.vgg_loss_and_grad(vgg_sd, x, y)
    got = P.pinned_backward(vgg_sd, saved, feats, 1.0, case[1:3])
    e_max, e_l2 = rel_errors(got, want)
    assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
    assert got.shape == x.shape and e_max <= 1e-12 and e_l2 <= 1e-12, (e_max, e_l2)


def test_forward_layers_and_prep_reference_are_the_oracle_in_float64(vgg_sd):
    """forward_layers of a float64 run's own tensors reproduces them; the prep reference is vgg_oracle.preprocess."""
    case = CASES[3]
    x, y = pair(*case)
    x0, saved, feats, _, _ = P.run_torch(vgg_sd, x, y, torch.float64)
    assert max(rel_errors(x0, P.prep_reference(torch.cat([x, y])))) <= 1e-13  # tap tables against F.interpolate
    for l, (got, want) in enumerate(zip(P.forward_layers(vgg_sd, x0[:case[0]], saved), saved)):
        assert max(rel_errors(got, want)) <= 1e-14, l
    assert torch.equal(F.max_pool2d(saved[15], 2, 2), feats[:case[0]])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_autograd_sits_on_its_own_pinned_backward(vgg_sd, case):
    """torch fp32 autograd against the float64 backward pinned to its own activations: <= 1e-5 in both metrics (measured
    1.3e-7 .. 6.7e-7; against the free float64 oracle the same gradients are 1e-2 away)."""
    r = _fp32_run(vgg_sd, case)
    e_max, e_l2 = rel_errors(r["dpred"], r["want"])
    print(f"{case}: fp32 autograd vs pinned float64 backward: max-rel {e_max:.2e} rel-L2 {e_l2:.2e}")
    assert e_max <= 1e-5 and e_l2 <= 1e-5, (e_max, e_l2)


# ---- mutations: one broken step in an otherwise exact backward ---------------------------------------------------------
class _BorderTap(P.Steps):
    """The last column of layer l's data gradient loses the tap of kernel column kx = 2 (its left neighbour's share)."""

    def __init__(self, l):
        self.l = l

    def conv_dgrad(self, l, g, w):
        out = F.conv_transpose2d(g, w, padding=1)
        if l == self.l:
            only = torch.zeros_like(w)
            only[..., 2] = w[..., 2]
            out[..., -1] -= F.conv_transpose2d(g, only, padding=1)[..., -1]
        return out


class _DroppedRowGetsGradient(P.Steps):
    """The row an odd pool drops is treated as a third row of the last window row (a missing `oy < OH`)."""

    def pool_adjoint(self, l, g, y):
        out = super().pool_adjoint(l, g, y)
        H, W = y.shape[-2:]
        if H % 2:
            k = P.pool_winners(y)[:, :, -1]                                    # (N, C, OW)
            for dx in (0, 1):
                out[:, :, H - 1, dx:2 * (W // 2):2] = g[:, :, -1] * (k == dx)  # slot (dy = 0, dx) of the clamped window
        return out


class _ClampedTapsOverwrite(P.Steps):
    """Forward taps that the clamp sends to one source index are stored, not added, in the transpose table."""

    def resize_adjoint(self, g, H, W):
        def matrix(n_in, n_out):
            idx, w = O.bicubic_taps(n_in, n_out)
            m = torch.zeros((n_out, n_in), dtype=g.dtype)
            for k in range(4):
                m[torch.arange(n_out), idx[:, k]] = w[:, k].to(g.dtype)
            return m
        return matrix(H, g.shape[-2]).t() @ (g @ matrix(W, g.shape[-1]))


class _PoolWithoutReluMask(P.Steps):
    """Layers in front of a pool skip their ReLU mask: the winner of an all-zero window passes its gradient on."""

    def relu_mask(self, l, g, y):
        return g if l in O.POOL_AFTER else super().relu_mask(l, g, y)


class _SeedOverBatch(P.Steps):
    def seed(self, fx, fy, grad_loss):
        return 2.0 * (fx - fy) / fx.shape[0] * grad_loss


C40, C224, C24 = CASES[0], CASES[2], CASES[3]
# (name, steps, case, visible, measured (max-rel, rel-L2) on the CPU with the seeded weights)
MUTATIONS = [
    ("conv1 border tap", _BorderTap(0), C40, True, (1.49e-1, 1.66e-2)),
    ("conv3 border tap", _BorderTap(2), C40, True, (1.08e-1, 2.28e-2)),
    ("conv10 border tap", _BorderTap(9), C40, True, (1.59e-1, 5.93e-2)),
    ("conv16 border tap", _BorderTap(15), C40, True, (1.46e-1, 8.74e-2)),
    ("conv1 border tap", _BorderTap(0), C224, True, (1.36e-1, 1.53e-2)),
    ("conv3 border tap", _BorderTap(2), C224, True, (1.41e-1, 2.37e-2)),
    ("conv10 border tap", _BorderTap(9), C224, True, (1.84e-1, 6.29e-2)),
    ("conv16 border tap", _BorderTap(15), C224, True, (1.79e-1, 1.03e-1)),
    ("dropped pool row (5 -> 2) gets gradient", _DroppedRowGetsGradient(), C40, True, (3.43e-1, 3.51e-1)),
    ("clamped bicubic taps overwrite", _ClampedTapsOverwrite(), C24, True, (1.03e-1, 1.29e-1)),
    ("pool without ReLU mask", _PoolWithoutReluMask(), C40, True, (1.80e+0, 1.95e+0)),
    ("seed / B instead of / numel", _SeedOverBatch(), C40, True, (3.58e+3, 3.58e+3)),
]


@pytest.mark.parametrize("name,steps,case,visible,measured", MUTATIONS,
                         ids=[f"{m[0].replace(' ', '_')}-{IDS[CASES.index(m[2])]}" for m in MUTATIONS])
def test_a_single_broken_step_is_far_outside_the_gpu_bar(vgg_sd, name, steps, case, visible, measured):
    r = _fp32_run(vgg_sd, case)
    got = P.pinned_backward(vgg_sd, r["saved"], r["feats"], GRAD_LOSS, case[1:3], steps=steps)
    e_max, e_l2 = rel_errors(got, r["want"])
    print(f"{name} {case}: max-rel {e_max:.2e} rel-L2 {e_l2:.2e}")
    if visible:
        assert max(e_max, e_l2) >= 10 * GPU_BAR_CEILING, (name, e_max, e_l2)
