"""CPU side of the MSE+Perceptual_noise loss: the prep kernel's resampling specification, weight loading, the channel check,
the C-ABI's shape checks and the loss selection of the trainers."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import vgg_oracle as O


@pytest.mark.parametrize("n", [64, 128, 200, 256, 512])
def test_bicubic_taps_match_interpolate(n):
    """The 4-tap tables the prep kernel reads reproduce F.interpolate(bicubic, align_corners=False) n -> 224, both axes."""
    from diffusionremotesensing_amd import synthetic
    img = synthetic.tensor_normal(f"vgg.taps.{n}", (2, 3, n, n + 8)).double()
    want = F.interpolate(img, size=(224, 224), mode="bicubic", align_corners=False)
    got = O.resize_by_taps(img, 224, 224)
    assert (got - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("n", [64, 200, 512])
def test_bicubic_adjoint_taps_match_autograd(n):
    """The transpose tables of the backward are the adjoint of the forward resize (autograd of F.interpolate)."""
    from diffusionremotesensing_amd import synthetic
    img = synthetic.tensor_normal(f"vgg.adj.{n}", (1, 3, n, n)).double().requires_grad_(True)
    g = synthetic.tensor_normal(f"vgg.adj.g.{n}", (1, 3, 224, 224)).double()
    F.interpolate(img, size=(224, 224), mode="bicubic", align_corners=False).backward(g)
    got = O.resize_adjoint_by_taps(g, n, n)
    assert (got - img.grad).abs().max().item() < 1e-10 * g.abs().max().item() * 16


def test_oracle_width_only_resize_and_odd_pooling():
    """A 200 x 224 input is not resized (the reference tests the width only) and pools to 6 x 7 features."""
    sd = O.seeded_vgg_state_dict()
    x = torch.zeros(1, 3, 200, 224, dtype=torch.float64)
    assert O.preprocess(x).shape == (1, 3, 200, 224)
    assert O.features(sd, O.preprocess(x)).shape == (1, 512, 6, 7)


def test_missing_checkpoint_names_the_path(tmp_path, monkeypatch):
    from diffusionremotesensing_amd import perceptual
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    want = os.path.join(str(tmp_path), "hub", "checkpoints", "vgg19-dcbb9e9d.pth")
    assert perceptual.checkpoint_path() == want
    with pytest.raises(FileNotFoundError) as e:
        perceptual.feature_weights()
    assert want in str(e.value)


def test_checkpoint_with_torchvision_layout_loads(tmp_path, monkeypatch):
    """A vgg19 state dict with features.* and classifier.* keys, saved where torchvision caches it, loads under TORCH_HOME."""
    from diffusionremotesensing_amd import perceptual
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    sd = O.seeded_vgg_state_dict(classifier=True)
    path = perceptual.checkpoint_path()
    os.makedirs(os.path.dirname(path))
    torch.save(sd, path)
    got = perceptual.feature_weights()
    assert len(got) == 16
    for (w, b), k in zip(got, perceptual.FEATURE_CONVS):
        assert torch.equal(w, sd[f"features.{k}.weight"]) and torch.equal(b, sd[f"features.{k}.bias"])
    # the features Sequential's own state dict (no "features." prefix) is accepted as well
    bare = {k[len("features."):]: v for k, v in sd.items() if k.startswith("features.")}
    assert all(torch.equal(a[0], b[0]) for a, b in zip(perceptual.feature_weights(bare), got))
    broken = dict(sd)
    broken["features.5.weight"] = broken["features.5.weight"][:, :32]
    with pytest.raises(ValueError, match="features.5"):
        perceptual.feature_weights(broken)


def test_one_channel_input_raises_like_the_reference():
    """C != 3: the reference's Normalize raises; so do the oracle and the port (before any GPU work)."""
    from diffusionremotesensing_amd.perceptual import VGGPerceptualLoss
    x = torch.zeros(2, 1, 64, 64)
    with pytest.raises(RuntimeError):
        O.vgg_loss(O.seeded_vgg_state_dict(), x.double(), x.double())
    loss = VGGPerceptualLoss.__new__(VGGPerceptualLoss)  # the channel check needs no weights and no device
    torch.nn.Module.__init__(loss)
    with pytest.raises(RuntimeError, match="3-channel"):
        loss(x, x)


def test_loss_selection(tmp_path, monkeypatch):
    """MSE+Perceptual_noise selects CombinedLoss(MSE, VGG, 0.3) in all three trainers: the SAR and generation trainers
    inherit the selection; without the checkpoint it fails with FileNotFoundError, not NotImplementedError."""
    from diffusionremotesensing_amd import perceptual
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as DS
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as DG
    for cls in (DS, DG):
        assert issubclass(cls, Diffusion) and "_loss_function" not in cls.__dict__
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="vgg19-dcbb9e9d.pth"):
        Diffusion._loss_function("MSE+Perceptual_noise", "cuda:0")
    c = perceptual.CombinedLoss(torch.nn.MSELoss(), torch.nn.L1Loss(), weight_first=0.3)
    p, t = torch.randn(2, 3, 4, 4), torch.randn(2, 3, 4, 4)
    want = 0.3 * F.mse_loss(p, t) + 0.7 * F.l1_loss(p, t)
    assert math.isclose(c(p, t).item(), want.item(), rel_tol=1e-6)


@pytest.mark.parametrize("H,W,ok", [(64, 64, True), (200, 224, True), (31, 224, False), (224, 224, True)])
def test_plan_shapes(H, W, ok):
    """drs_vgg_plan_create takes every shape whose 224-wide feature stack is non-empty and sizes its buffers; the width
    decides the resize."""
    import ctypes as C
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for impl in (_lib.IMPL_MFMA_F32, _lib.IMPL_MFMA_BF16X3):
        st = lib.drs_vgg_plan_create(C.byref(h), 2, H, W, impl)
        assert (st == 0) == ok, lib.drs_last_error()
        if ok:
            H0 = 224 if W != 224 else H
            assert lib.drs_vgg_workspace_bytes(h) > 2 * 2 * H0 * 224 * 64 * 4
            assert lib.drs_vgg_packed_bytes(h) > 20e6 * 4
            lib.drs_vgg_plan_destroy(h)
    assert lib.drs_vgg_plan_create(C.byref(h), 2, 64, 64, _lib.IMPL_DIRECT) == 1  # no direct-kernel VGG


def test_plan_tensor_table():
    """drs_vgg_num_tensors / _tensor_name / _tensor_shape: x0 with its pad channel, the 16 saved prediction-half ReLU outputs
    at their (floor-halved) level sizes, the features of both halves; the saved tensors are refused before a forward with
    save = 1, and a bad index or null pointer before anything runs."""
    import ctypes as C
    from diffusionremotesensing_amd import _lib
    from diffusionremotesensing_amd.perceptual import FEATURE_CHANNELS
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.drs_vgg_num_tensors(None) == 0 and lib.drs_vgg_tensor_name(None, 0) is None
    assert lib.drs_vgg_plan_create(C.byref(h), 3, 72, 224, _lib.IMPL_MFMA_F32) == 0, lib.drs_last_error()
    names = [lib.drs_vgg_tensor_name(h, i).decode() for i in range(lib.drs_vgg_num_tensors(h))]
    assert names == ["x0"] + [f"conv{l}" for l in range(1, 17)] + ["features"]
    assert lib.drs_vgg_tensor_name(h, 18) is None and lib.drs_vgg_tensor_name(h, -1) is None

    def shape(i):
        d = [C.c_int() for _ in range(4)]
        assert lib.drs_vgg_tensor_shape(h, i, *[C.byref(v) for v in d]) == 0
        return tuple(v.value for v in d)
    level = (0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4)
    assert shape(0) == (6, 4, 72, 224)
    assert [shape(1 + l) for l in range(16)] == [(3, FEATURE_CHANNELS[l], 72 >> level[l], 224 >> level[l]) for l in range(16)]
    assert shape(9) == (3, 512, 9, 28) and shape(17) == (6, 512, 2, 7)
    d = C.c_int()
    assert lib.drs_vgg_tensor_shape(h, 18, *[C.byref(d)] * 4) == 1 and lib.drs_vgg_tensor_shape(h, 0, None, None, None, None) == 1
    fake = C.c_void_p(256)  # never dereferenced: every call below is refused first
    assert lib.drs_vgg_read_tensor(h, 18, fake, fake, None) == 1
    assert lib.drs_vgg_read_tensor(h, 0, None, fake, None) == 1 and lib.drs_vgg_read_tensor(h, 0, fake, None, None) == 1
    for i in range(1, 17):
        assert lib.drs_vgg_read_tensor(h, i, fake, fake, None) == 5 and b"save = 1" in lib.drs_last_error()
    lib.drs_vgg_plan_destroy(h)
