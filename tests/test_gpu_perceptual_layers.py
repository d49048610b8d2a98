"""The VGG19 perceptual loss (csrc/vgg_loss.hip) layer by layer on the GPU, with every ReLU mask and max-pool winner pinned
to the device's own run (tests/vgg_pinned.py), for both DRS_VGG_IMPL values.

tests/test_gpu_perceptual.py compares loss and dpred with a free float64 oracle, whose near-tie flips force bars of 2e-2 /
0.15 (5e-2 / 0.3 on mfma_bf16x3); a data-gradient convolution that drops a border tap passes them
(tests/test_vgg_pinned_host.py measures such mutations at 1.5e-2 .. 3.5e-1).  Here every tensor of the plan
(drs_vgg_read_tensor) is held to a float64 reference of the ONE operation that made it, fed the device's own inputs:

  prep       x0[:, :3] against float64 F.interpolate + Normalize at test_bicubic's 1e-5; the pad channel is exactly 0
  conv1..16  against relu(conv2d_f64(the device's previous tensor)) at the operator bars 2e-5 (mfma_f32) / 1e-4 (mfma_bf16x3),
             first / last row and column also on their own scale
  pools      features is bit-equal to F.max_pool2d of conv16; pool1 .. pool4 write into the ping-pong buffers the next layer
             overwrites, so they are judged through the convolution behind them, whose reference input is F.max_pool2d of
             the saved tensor in front of the pool
  target     the same pair with prediction and target swapped: features of each image at 1e-6 of its value in the other
             batch position, the swapped run's conv1..16 under the per-layer check too
  loss       the float64 mean of (features[:B] - features[B:])^2 of the device's own features, to 2e-7
  backward   dpred of (0.7 * loss).backward() against pinned_backward(grad_loss = 0.7)

dpred bars (DPRED_BARS): 4 x the worst figure measured on the MI355X (the kernels are deterministic: the margin is for
other inputs), and never above 1e-3, a tenth of the smallest mutation effect.  Measured max-rel / rel-L2, in CASES order:
  mfma_f32      2.02e-6 / 2.24e-6, 2.35e-6 / 2.40e-6, 2.28e-6 / 2.45e-6, 3.69e-7 / 1.76e-6, 2.36e-6 / 2.42e-6, 2.26e-6 / 2.15e-6
  mfma_bf16x3   1.60e-5 / 1.71e-5, 1.56e-5 / 1.70e-5, 1.64e-5 / 1.70e-5, 3.68e-6 / 1.28e-5, 1.57e-5 / 1.70e-5, 1.74e-5 / 1.61e-5
(torch fp32 on the CPU against the same reference: 6e-7.)  The other figures of the same runs: prep 1.0e-7 .. 1.6e-7, worst
layer (borders included) 2.8e-6 on mfma_f32 and 9.1e-6 on mfma_bf16x3, swapped batch positions bit-equal, loss 8e-9 .. 6e-8.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import vgg_oracle as O
import vgg_pinned as P
from conftest import rel_errors

pytestmark = pytest.mark.gpu

TOL = {"mfma_f32": 2e-5, "mfma_bf16x3": 1e-4}  # tests/test_gpu_parity.py TOL_F32 / TOL_BF16X3
TOL_PREP = 1e-5                                # tests/test_gpu_parity.py test_bicubic
TOL_BATCH = 1e-6                               # tests/test_gpu_parity.py batch independence
TOL_LOSS = 2e-7                                # fp64 sum on the device, rounded once to fp32 (6e-8)
DPRED_BAR_CEILING = 1e-3
DPRED_BARS = {"mfma_f32": 4 * 2.453e-6, "mfma_bf16x3": 4 * 1.737e-5}  # 4 x the worst measured figure (module docstring)
GRAD_LOSS = 0.7
# (B, H, W, near).  40 x 224: no resize, levels 40 / 20 / 10 on the wave-specialised kernel and 5 / 2 on the <= 8-row generic
# path, pool 5 -> 2 drops a row.  3 x 72 x 224: odd batch (6 images, save-copy offset), 9 -> 4.  224 x 224: the production
# size at every level.  24 x 40: resize up, non-square, clamped taps on all four borders.  300 x 260: resize down.
# near: y = x + 0.05 n, a small seed.
CASES = [(1, 40, 224, False), (3, 72, 224, False), (1, 224, 224, False), (1, 24, 40, False), (1, 300, 260, False),
         (2, 40, 224, True)]
IDS = [f"B{c[0]}_{c[1]}x{c[2]}{'_near' if c[3] else ''}" for c in CASES]
EDGES = {"row0": (..., slice(0, 1), slice(None)), "row-1": (..., slice(-1, None), slice(None)),
         "col0": (..., slice(0, 1)), "col-1": (..., slice(-1, None))}
_MEASURED = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def vgg_sd():
    return O.seeded_vgg_state_dict()


def _pair(B, H, W, near):
    from diffusionremotesensing_amd import synthetic
    x = synthetic.tensor_normal(f"vggl.x.{B}.{H}.{W}", (B, 3, H, W))
    if near:
        return x, x + 0.05 * synthetic.tensor_normal(f"vggl.n.{B}.{H}.{W}", (B, 3, H, W))
    return x, synthetic.tensor_normal(f"vggl.y.{B}.{H}.{W}", (B, 3, H, W))


def _device_run(loss_fn, dev, x, y, backward):
    """One forward (and backward of GRAD_LOSS * loss): the plan's tensors, the loss and dpred, on the CPU."""
    xd = x.to(dev).requires_grad_(True)
    loss = loss_fn(xd, y.to(dev))
    plan = loss_fn._plan(*x.shape[:1], *x.shape[2:])
    t = {name: plan.read_tensor(name).cpu() for name in plan.tensor_names()}
    dpred = None
    if backward:
        (GRAD_LOSS * loss).backward()
        dpred = xd.grad.detach().cpu()
    return dict(loss=loss.item(), x0=t["x0"], features=t["features"], saved=[t[f"conv{l + 1}"] for l in range(16)],
                dpred=dpred)


def _layer_errors(sd, run, B):
    """Per layer: the worst of (max-rel, rel-L2) of the whole tensor and of each border line on its own scale."""
    want = P.forward_layers(sd, run["x0"][:B, :3], run["saved"])
    out = []
    for got, ref in zip(run["saved"], want):
        errs = {"all": max(rel_errors(got, ref))}
        errs.update({k: max(rel_errors(got[sl], ref[sl])) for k, sl in EDGES.items()})
        out.append(errs)
    return out


def _measure(dev, sd, case, impl):
    """Everything the tests below assert on, as numbers: one device run per (case, impl) and one pass over its references
    (the tensors of a 224 x 224 run are not kept)."""
    if (case, impl) in _MEASURED:
        return _MEASURED[case, impl]
    from diffusionremotesensing_amd.perceptual import VGGPerceptualLoss
    B, H, W, _ = case
    x, y = _pair(*case)
    old = os.environ.get("DRS_VGG_IMPL")
    os.environ["DRS_VGG_IMPL"] = impl
    try:
        loss_fn = VGGPerceptualLoss(dev, state_dict=sd)
        run = _device_run(loss_fn, dev, x, y, backward=True)
        swp = _device_run(loss_fn, dev, y, x, backward=False)
    finally:
        if old is None:
            del os.environ["DRS_VGG_IMPL"]
        else:
            os.environ["DRS_VGG_IMPL"] = old
    m = {}
    m["shapes_ok"] = (run["x0"].shape[:2] == (2 * B, 4) and run["features"].shape[:2] == (2 * B, 512)
                      and all(t.shape[0] == B for t in run["saved"]) and run["dpred"].shape == x.shape)
    m["prep"] = rel_errors(run["x0"][:, :3], P.prep_reference(torch.cat([x, y])))
    m["pad_is_zero"] = bool((run["x0"][:, 3] == 0).all()) and bool((swp["x0"][:, 3] == 0).all())
    m["layers"] = _layer_errors(sd, run, B)
    m["layers_swapped"] = _layer_errors(sd, swp, B)
    m["pool_bit_equal"] = (torch.equal(run["features"][:B], F.max_pool2d(run["saved"][15], 2, 2))
                           and torch.equal(swp["features"][:B], F.max_pool2d(swp["saved"][15], 2, 2)))
    f, g = run["features"], swp["features"]
    m["batch"] = max(max(rel_errors(g[B + i], f[i]) + rel_errors(g[i], f[B + i])) for i in range(B))
    want_loss = torch.mean((f[:B].double() - f[B:].double()) ** 2).item()
    m["loss"] = abs(run["loss"] - want_loss) / want_loss
    m["dpred"] = rel_errors(run["dpred"], P.pinned_backward(sd, run["saved"], f, GRAD_LOSS, (H, W)))
    print(f"{impl} {case}: prep {m['prep'][0]:.2e}/{m['prep'][1]:.2e}  worst layer "
          f"{max(max(e.values()) for e in m['layers'] + m['layers_swapped']):.2e}  batch {m['batch']:.2e}  "
          f"loss {m['loss']:.2e}  dpred max-rel {m['dpred'][0]:.3e} rel-L2 {m['dpred'][1]:.3e}")
    _MEASURED[case, impl] = m
    return m


both = pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
cases = pytest.mark.parametrize("case", CASES, ids=IDS)


@both
@cases
def test_prep(dev, vgg_sd, case, impl):
    m = _measure(dev, vgg_sd, case, impl)
    assert m["shapes_ok"] and m["pad_is_zero"]
    assert max(m["prep"]) <= TOL_PREP, m["prep"]


@both
@cases
def test_every_conv(dev, vgg_sd, case, impl):
    m = _measure(dev, vgg_sd, case, impl)
    bad = {f"conv{l + 1}.{k}": f"{v:.2e}" for l, errs in enumerate(m["layers"]) for k, v in errs.items() if not v <= TOL[impl]}
    assert not bad, bad


@both
@cases
def test_pools(dev, vgg_sd, case, impl):
    assert _measure(dev, vgg_sd, case, impl)["pool_bit_equal"]


@both
@cases
def test_target_half(dev, vgg_sd, case, impl):
    m = _measure(dev, vgg_sd, case, impl)
    assert m["batch"] <= TOL_BATCH, m["batch"]
    bad = {f"conv{l + 1}.{k}": f"{v:.2e}" for l, errs in enumerate(m["layers_swapped"]) for k, v in errs.items()
           if not v <= TOL[impl]}
    assert not bad, bad


@both
@cases
def test_loss(dev, vgg_sd, case, impl):
    m = _measure(dev, vgg_sd, case, impl)
    assert m["loss"] <= TOL_LOSS, m["loss"]


@both
@cases
def test_backward(dev, vgg_sd, case, impl):
    m = _measure(dev, vgg_sd, case, impl)
    assert DPRED_BARS[impl] <= DPRED_BAR_CEILING
    e_max, e_l2 = m["dpred"]
    assert e_max <= DPRED_BARS[impl] and e_l2 <= DPRED_BARS[impl], (e_max, e_l2)
