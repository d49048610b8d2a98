"""The MSE+Perceptual_noise loss on the GPU (csrc/vgg_loss.hip through diffusionremotesensing_amd/perceptual.py): loss value
and d(loss)/d(pred) against the float64 oracle (tests/vgg_oracle.py) for both DRS_VGG_IMPL values, determinism, one
training step's UNet gradients against the float64 oracle with the combined loss, and the three trainers' loops.

Bars: loss relative error <= 1e-4 for both arithmetics.  dpred (conftest.rel_errors): the loss is piecewise linear in its
ReLU masks and max-pool choices, and a near-tie that rounding decides otherwise than float64 does sends one gradient
element to a neighbouring pixel; a handful of such flips over 16 layers cost up to 1.5e-2 rel-L2 and 1e-1 max-rel in ANY
fp32 evaluation (torch's own fp32 run of this oracle on the CPU, same cases: 9e-4 - 1.5e-2 rel-L2, 1e-2 - 9.9e-2 max-rel).
So dpred is held to rel-L2 <= 2e-2 and max-rel <= 0.15 on exact fp32 (mfma_f32, the default) and to the project's
split-bf16 gradient bar rel-L2 <= 5e-2 (grad_check.REL_L2_BF16X3), max-rel <= 0.3 on mfma_bf16x3.  Measured in DESIGN.md
section 9."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import vgg_oracle as O
from conftest import rel_errors

pytestmark = pytest.mark.gpu

LOSS_REL = 1e-4
DPRED_BARS = {"mfma_f32": (2e-2, 0.15), "mfma_bf16x3": (5e-2, 0.3)}  # (rel-L2, max-rel)
# (B, H, W, near): 64^2 upsamples, 256^2 downsamples, 224^2 is not resized, 200 x 224 is not resized and pools oddly;
# near = a near-converged pair y = x + 0.05 n
CASES = [(1, 64, 64, False), (2, 256, 256, False), (5, 224, 224, False), (2, 200, 224, False), (2, 64, 64, True),
         (2, 224, 224, True)]
_ORACLE = {}


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
    x = synthetic.tensor_normal(f"vgg.x.{B}.{H}.{W}", (B, 3, H, W))
    if near:
        y = x + 0.05 * synthetic.tensor_normal(f"vgg.n.{B}.{H}.{W}", (B, 3, H, W))
    else:
        y = synthetic.tensor_normal(f"vgg.y.{B}.{H}.{W}", (B, 3, H, W))
    return x, y


def _oracle(sd, case):
    if case not in _ORACLE:
        _ORACLE[case] = O.vgg_loss_and_grad(sd, *_pair(*case))
    return _ORACLE[case]


def _run(dev, sd, x, y, impl, monkeypatch):
    from diffusionremotesensing_amd.perceptual import VGGPerceptualLoss
    monkeypatch.setenv("DRS_VGG_IMPL", impl)
    loss_fn = VGGPerceptualLoss(dev, state_dict=sd)
    xd = x.to(dev).requires_grad_(True)
    loss = loss_fn(xd, y.to(dev))
    loss.backward()
    return loss.detach().cpu().item(), xd.grad.detach().cpu(), loss_fn


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"B{c[0]}_{c[1]}x{c[2]}{'_near' if c[3] else ''}")
def test_loss_and_dpred_vs_oracle(dev, vgg_sd, case, impl, monkeypatch):
    x, y = _pair(*case)
    want_loss, want_grad = _oracle(vgg_sd, case)
    got_loss, got_grad, _ = _run(dev, vgg_sd, x, y, impl, monkeypatch)
    e_loss = abs(got_loss - want_loss) / abs(want_loss)
    e_max, e_l2 = rel_errors(got_grad, want_grad)
    print(f"{impl} {case}: loss {want_loss:.6e} rel {e_loss:.2e}; dpred max-rel {e_max:.2e} rel-L2 {e_l2:.2e}")
    assert got_grad.shape == x.shape
    bar_l2, bar_max = DPRED_BARS[impl]
    assert e_loss <= LOSS_REL and e_l2 <= bar_l2 and e_max <= bar_max, (e_loss, e_max, e_l2)


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
def test_no_grad_forward_matches_and_saves_nothing(dev, vgg_sd, impl, monkeypatch):
    """Under torch.no_grad (the validation loop) the loss is the same number and carries no graph."""
    x, y = _pair(2, 64, 64, False)
    got_loss, _, loss_fn = _run(dev, vgg_sd, x, y, impl, monkeypatch)
    with torch.no_grad():
        v = loss_fn(x.to(dev), y.to(dev))
    assert v.grad_fn is None and v.dim() == 0 and v.is_cuda
    assert v.item() == got_loss


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
def test_deterministic(dev, vgg_sd, impl, monkeypatch):
    x, y = _pair(2, 256, 256, False)
    a = _run(dev, vgg_sd, x, y, impl, monkeypatch)
    b = _run(dev, vgg_sd, x, y, impl, monkeypatch)
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_train_step_grads_vs_oracle(dev, seeded_sd, vgg_sd):
    """Diffusion.train_step with CombinedLoss(MSE, VGG, 0.3): every UNet parameter gradient against a float64 oracle step
    with the same batch, timesteps and noise (captured from the step) and the combined loss."""
    from diffusionremotesensing_amd.perceptual import CombinedLoss, VGGPerceptualLoss
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from diffusionremotesensing_amd import synthetic
    from grad_check import MAX_REL_F32, REL_L2_F32, check_grads, model_grads
    from perceptual_grad_check import oracle_step_combined
    torch.manual_seed(0)
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).train()
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=1500, device=dev, magnification_factor=2,
                  image_size=32, Degradation_type="DownBlur")
    cap = {}
    noise_images = d.noise_images

    def capture(x, t):
        x_t, n = noise_images(x, t)
        cap.update(x_t=x_t.detach().cpu(), t=t.detach().cpu(), noise=n.detach().cpu())
        return x_t, n
    d.noise_images = capture
    loss_fn = CombinedLoss(torch.nn.MSELoss(), VGGPerceptualLoss(dev, state_dict=vgg_sd), weight_first=0.3)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    hr = synthetic.tensor_uniform("vgg.step.hr", (2, 3, 32, 32))
    lr = synthetic.tensor_uniform("vgg.step.lr", (2, 3, 16, 16))
    loss = d.train_step(m, opt, loss_fn, lr, hr)
    torch.cuda.synchronize()
    got = model_grads(m)
    args = (seeded_sd, vgg_sd, list(got), cap["x_t"], cap["t"], lr, cap["noise"])
    ref_loss, ref = oracle_step_combined(*args, mag=2)
    assert abs(loss.item() - ref_loss) <= 1e-4 * abs(ref_loss), (loss.item(), ref_loss)
    # 10 x check_grads' fp32 bars: the ReLU / max-pool flips of the VGG term (module docstring) reach every UNet gradient
    # through d(loss)/d(pred) (measured: worst rel-L2 1.7e-3, max-rel 2.7e-3)
    check_grads(got, ref, 10 * REL_L2_F32, 10 * MAX_REL_F32, what="train_step MSE+Perceptual_noise")


def _fake_checkpoint(tmp_path, monkeypatch):
    from diffusionremotesensing_amd import perceptual
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    path = perceptual.checkpoint_path()
    os.makedirs(os.path.dirname(path))
    torch.save(O.seeded_vgg_state_dict(classifier=True), path)


def test_trainers_run_the_loss(dev, seeded_sd, seeded_sd_gen, seeded_sd_sar, tmp_path, monkeypatch):
    """One epoch of Diffusion.train with loss=MSE+Perceptual_noise and EMA, the weights from the torch hub cache: superres
    and generation train and validate (finite losses, snapshot written); SAR->NDVI (1 output channel) raises the channel
    error like the reference."""
    from torch.utils.data import DataLoader
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion, SyntheticSuperresDataset
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as DG, SyntheticClassDataset
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as DS, SyntheticSarNdviDataset
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    _fake_checkpoint(tmp_path, monkeypatch)
    torch.manual_seed(0)
    # superres: 6 training patches in batches of 4 (a last batch of 2: a second plan), validation on 4
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev)
    snap = str(tmp_path / "superres.pt")
    d = Diffusion("cosine", m, snap, noise_steps=50, device=dev, magnification_factor=2, image_size=32,
                  Degradation_type="DownBlur", ema_smoothing=True)
    ds = SyntheticSuperresDataset(6, 3, 32, 2, seed=5)
    val = torch.utils.data.Subset(ds, range(4))
    losses = []
    orig = d.train_step

    def step(*a, **k):
        out = orig(*a, **k)
        losses.append(out.detach())
        return out
    d.train_step = step
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=DataLoader(ds, batch_size=4, shuffle=False),
            val_loader=DataLoader(val, batch_size=4, shuffle=False), patience=5, loss="MSE+Perceptual_noise", verbose=False)
    assert len(losses) == 2 and all(math.isfinite(v.item()) for v in losses)
    assert os.path.exists(snap) and len(torch.load(snap)["MODEL_STATE"]) == 299
    # generation
    g = Residual_Attention_UNet_generation(3, 3, 10, dev)
    g.load_state_dict(seeded_sd_gen)
    g = g.to(dev)
    dg = DG("cosine", g, str(tmp_path / "gen.pt"), noise_steps=50, device=dev, image_size=32, ema_smoothing=True)
    gds = SyntheticClassDataset(4, 3, 32, 10, seed=3)
    dg.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=DataLoader(gds, batch_size=4, shuffle=False),
             val_loader=DataLoader(gds, batch_size=4, shuffle=False), patience=5, loss="MSE+Perceptual_noise",
             verbose=False)
    assert os.path.exists(dg.snapshot_path)
    # SAR -> NDVI: one output channel
    s = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    s.load_state_dict(seeded_sd_sar)
    s = s.to(dev)
    dsr = DS("cosine", s, str(tmp_path / "sar.pt"), noise_steps=50, device=dev, image_size=32)
    sds = SyntheticSarNdviDataset(4, 2, 1, 32, seed=3)
    with pytest.raises(RuntimeError, match="3-channel"):
        dsr.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=DataLoader(sds, batch_size=4, shuffle=False),
                  val_loader=None, patience=5, loss="MSE+Perceptual_noise", verbose=False)
