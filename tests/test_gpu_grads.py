"""One training step of the HIP path (train-mode forward, MSE against seeded noise, loss.backward() through the C-ABI),
every live parameter's gradient compared element-wise with the float64 oracle's autograd on the same batch
(tests/grad_check.py), plus the updated running statistics of every BatchNorm.

The shapes reach the branches the golden shapes (B=4 32x32 x2, B=16 256x256 x2) do not: BatchNorm over one image, a
bottleneck of exactly 8 rows (plan.hip keeps the SP copy of dZ for levels with hh > 8) and of 9, the x3 / x4 bicubic
adjoints, odd and rectangular batches, partial tiles at every level, the SAR wiring, a class label that appears twice.
Every case has lr batch == batch (the backward requires it); the timesteps include 1 and T-1 = 1499.

Bars (grad_check.py): the training default (mfma_f32 forward, split-bf16 backward products), mfma_f32 and direct hold
rel-L2 <= 1e-3 and max-rel <= 5e-3 on every tensor; opt-in split-bf16 training rel-L2 <= 5e-2.

Measured on MI355X (worst tensor of each case, rel-L2 = max-rel for the 1-element ones):
  G5 direct 5.8e-6 (LR_encoder.blocks.0.conv2.bias), mfma_f32 3.6e-5 (attention_blocks.2.psi.0.bias),
  mfma_bf16x3 1.4e-2 rel-L2 (conv_blocks.0.batch_norm1.weight) / 3.3e-2 max-rel (conv_blocks.0.conv2.0.weight);
  single-image 7.0e-5, tall 5.8e-5, wide 2.6e-4, tiny 6.2e-5, SAR 1.3e-4, generation 6.8e-4 / unconditional 3.9e-5.
The largest are the psi biases: one scalar, the sum of d(psi_pre) over every pixel of a gate, and that sum cancels
(sum |terms| / |sum| = 518 for attention_blocks.0 in the generation case; the fp64 oracle shows it).  The fp32-vs-fp64
gap of the CPU oracle is at most 4.5e-5 on every case here.  Prediction and running statistics: at most 2e-6 and 2e-7
(1.9e-5 and 1.6e-6 on split bf16)."""
import os

import pytest
import torch

from conftest import golden_inputs
from grad_check import MAX_REL_F32, REL_L2_BF16X3, REL_L2_F32, check_grads
from train_step import build_model as _model, step as _step  # noqa: F401 (_model: used by test_gpu_guard.py)

pytestmark = pytest.mark.gpu

IMPLS = [i for i in os.environ.get("DRS_TEST_IMPLS", "direct,mfma_f32,mfma_bf16x3").split(",") if i]
T_MAX = 1499


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _bars(impl):
    return (REL_L2_BF16X3, None) if impl == "mfma_bf16x3" else (REL_L2_F32, MAX_REL_F32)


@pytest.mark.parametrize("impl", IMPLS)
def test_grads_g5(dev, seeded_sd, impl):
    """The golden training-step batch (G5: B=4, 32x32, x2) on every train plan."""
    from diffusionremotesensing_amd import synthetic
    x, t, lr = golden_inputs("g5", 4, 4, 3, 32, 2, 1500)
    noise = synthetic.tensor_normal("g5.noise", (4, 3, 32, 32))
    got, ref = _step(dev, "superres", seeded_sd, x, t, lr, noise, 2, train_impl=impl)
    check_grads(got, ref, *_bars(impl), what=f"G5 [{impl}]")


SUPERRES_CASES = [
    # (id, B, H, W, mag, timesteps)
    ("single-image", 1, 64, 64, 4, [1]),               # BN over one image; bottleneck exactly 8x8; x4 adjoint
    ("tall", 3, 72, 48, 3, [1, 700, T_MAX]),           # bottleneck 9x6; x3 adjoint; odd batch; rectangular
    ("wide", 2, 48, 72, 4, [T_MAX, 1]),                # bottleneck 6x9
    ("tiny", 2, 24, 40, 2, [1, T_MAX]),                # 3x5 bottleneck; partial tiles at every level
]


@pytest.mark.parametrize("case", SUPERRES_CASES, ids=[c[0] for c in SUPERRES_CASES])
def test_grads_superres_shapes(dev, seeded_sd, case):
    from diffusionremotesensing_amd import synthetic
    tag, B, H, W, mag, ts = case
    x = synthetic.tensor_normal(f"grads.{tag}.x", (B, 3, H, W))
    lr = synthetic.tensor_uniform(f"grads.{tag}.lr", (B, 3, H // mag, W // mag))
    noise = synthetic.tensor_normal(f"grads.{tag}.noise", (B, 3, H, W))
    got, ref = _step(dev, "superres", seeded_sd, x, torch.tensor(ts), lr, noise, mag)
    check_grads(got, ref, REL_L2_F32, MAX_REL_F32, f"{tag} B={B} {H}x{W} x{mag}")


def test_grads_sar(dev, seeded_sd_sar):
    """SAR->NDVI: conv_SAR_img, the SAR encoder at full resolution, one output channel."""
    from diffusionremotesensing_amd import synthetic
    x = synthetic.tensor_normal("grads.sar.x", (2, 1, 40, 24))
    sar = synthetic.tensor_uniform("grads.sar.sar", (2, 2, 40, 24))
    noise = synthetic.tensor_normal("grads.sar.noise", (2, 1, 40, 24))
    got, ref = _step(dev, "sar", seeded_sd_sar, x, torch.tensor([T_MAX, 1]), sar, noise)
    check_grads(got, ref, REL_L2_F32, MAX_REL_F32, "SAR B=2 40x24")


@pytest.mark.parametrize("labels", [[4, 9, 4], None], ids=["repeated-label", "unconditional"])
def test_grads_generation(dev, seeded_sd_gen, labels):
    """Class 4 twice in one batch: its label_emb row accumulates both images' gradients.  Unconditional: no gradient for
    the label embedding at all (grad None, like autograd)."""
    from diffusionremotesensing_amd import synthetic
    x = synthetic.tensor_normal("grads.gen.x", (3, 3, 24, 40))
    noise = synthetic.tensor_normal("grads.gen.noise", (3, 3, 24, 40))
    y = None if labels is None else torch.tensor(labels)
    got, ref = _step(dev, "generation", seeded_sd_gen, x, torch.tensor([1, 800, T_MAX]), y, noise)
    if labels is None:
        assert got["label_emb.weight"] is None and ref["label_emb.weight"] is None
    else:
        g = got["label_emb.weight"]
        assert g[[0, 1, 2, 3, 5, 6, 7, 8]].abs().max().item() == 0.0, "rows of absent classes must stay zero"
    check_grads(got, ref, REL_L2_F32, MAX_REL_F32, f"generation B=3 24x40 labels={labels}")
