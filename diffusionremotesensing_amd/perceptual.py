"""The MSE+Perceptual_noise training loss (reference train_diffusion_superres.py:25-77, selected at :353-356).

`VGGPerceptualLoss(x, y) = mean((F(P(x)) - F(P(y)))**2)` with F = torchvision's `vgg19().features` and P = bicubic resize to
224 x 224 (only when the width is not 224) + ImageNet normalisation, all of it in HIP (csrc/vgg_loss.hip, include/drs_hip.h
drs_vgg_*): prediction and target run as one batched forward, the backward returns d(loss)/d(prediction).  The VGG weights
are frozen, as in the reference; they come from torchvision's checkpoint file in the torch hub cache (nothing is downloaded)
or from a state dict given explicitly.

DRS_VGG_IMPL picks the arithmetic of the convolutions: `mfma_f32` (exact fp32 products, the default: DESIGN.md section 9)
or `mfma_bf16x3` (operands split into bf16 hi + lo).
"""
import ctypes as C
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib

# torchvision VGG19_Weights.IMAGENET1K_V1 (= VGG19_Weights.DEFAULT), as torchvision caches it
CHECKPOINT_NAME = "vgg19-dcbb9e9d.pth"
# indices of the convolutions in vgg19().features (cfg 64,64,M,128,128,M,256x4,M,512x4,M,512x4,M; a ReLU after each conv)
FEATURE_CONVS = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34)
FEATURE_CHANNELS = (64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512)
DEFAULT_IMPL = "mfma_f32"
_IMPLS = ("mfma_f32", "mfma_bf16x3")
_MAX_PLANS = 4  # (batch, height, width, impl) plans kept; each owns its packed weights and workspace


def checkpoint_path():
    """Where torchvision keeps VGG19_Weights.DEFAULT: <torch.hub.get_dir()>/checkpoints/vgg19-dcbb9e9d.pth."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", CHECKPOINT_NAME)


def vgg_impl():
    impl = os.environ.get("DRS_VGG_IMPL", DEFAULT_IMPL)
    if impl not in _IMPLS:
        raise ValueError(f"DRS_VGG_IMPL={impl!r}: expected one of {', '.join(_IMPLS)}")
    return impl


def feature_weights(state_dict=None):
    """[(weight, bias)] * 16 of vgg19().features, fp32 on the CPU.  `state_dict`: torchvision's layout
    (`features.{k}.weight` ..., `classifier.*` ignored) or that of the features Sequential alone (`{k}.weight`); None loads
    the checkpoint from the torch hub cache."""
    if state_dict is None:
        path = checkpoint_path()
        if not os.path.exists(path):
            raise FileNotFoundError(
                f"VGG19 weights not found at {path}. MSE+Perceptual_noise uses torchvision's VGG19_Weights.DEFAULT "
                f"(IMAGENET1K_V1) and downloads nothing: copy {CHECKPOINT_NAME} into {os.path.dirname(path)} (set TORCH_HOME "
                "to use another cache), or pass the state dict to VGGPerceptualLoss(device, state_dict=...).")
        state_dict = torch.load(path, map_location="cpu", weights_only=True)
    prefix = "features." if any(k.startswith("features.") for k in state_dict) else ""
    out = []
    for k, cout in zip(FEATURE_CONVS, FEATURE_CHANNELS):
        cin = 3 if not out else out[-1][0].shape[0]
        try:
            w, b = state_dict[f"{prefix}{k}.weight"], state_dict[f"{prefix}{k}.bias"]
        except KeyError as e:
            raise KeyError(f"VGG19 state dict has no {e.args[0]!r}: expected torchvision's vgg19 key layout") from None
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise ValueError(f"VGG19 features.{k}: weight {tuple(w.shape)} / bias {tuple(b.shape)}, expected "
                             f"({cout}, {cin}, 3, 3) / ({cout},)")
        out.append((w.detach().float().contiguous(), b.detach().float().contiguous()))
    return out


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Plan:
    """One drs_vgg_plan with its packed weights and workspace."""

    def __init__(self, lib, params, B, H, W, impl, device):
        self.lib, self.device = lib, device
        h = C.c_void_p()
        _lib.check(lib.drs_vgg_plan_create(C.byref(h), B, H, W, _lib.IMPL_BY_NAME[impl]), "drs_vgg_plan_create")
        self.handle = h
        self.packed_bytes = lib.drs_vgg_packed_bytes(h)
        self.ws_bytes = lib.drs_vgg_workspace_bytes(h)
        self.packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=device)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        ptrs = (C.c_void_p * len(params))(*[t.data_ptr() for t in params])
        with torch.cuda.device(device):
            _lib.check(lib.drs_vgg_pack_weights(h, ptrs, C.c_void_p(self.packed.data_ptr()), self.packed_bytes,
                                                _stream(device)), "drs_vgg_pack_weights")
        self.generation = 0  # forwards run; a backward must belong to the latest forward (the workspace holds only that one)

    def forward(self, pred, target, save):
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.drs_vgg_forward(self.handle, C.c_void_p(self.packed.data_ptr()), C.c_void_p(pred.data_ptr()),
                                                C.c_void_p(target.data_ptr()), C.c_void_p(loss.data_ptr()), int(save),
                                                C.c_void_p(self.workspace.data_ptr()), self.ws_bytes, _stream(self.device)),
                       "drs_vgg_forward")
        self.generation += 1
        return loss

    def backward(self, grad_loss, dpred):
        with torch.cuda.device(self.device):
            _lib.check(self.lib.drs_vgg_backward(self.handle, C.c_void_p(self.packed.data_ptr()),
                                                 C.c_void_p(grad_loss.data_ptr()), C.c_void_p(dpred.data_ptr()),
                                                 C.c_void_p(self.workspace.data_ptr()), self.ws_bytes,
                                                 _stream(self.device)), "drs_vgg_backward")

    def tensor_names(self):
        """Names of the tensors the last forward left in the workspace: x0, conv1 .. conv16 (save=True only), features."""
        return [self.lib.drs_vgg_tensor_name(self.handle, i).decode() for i in range(self.lib.drs_vgg_num_tensors(self.handle))]

    def read_tensor(self, name):
        """One workspace tensor of the last forward as an NCHW fp32 device tensor (include/drs_hip.h drs_vgg_read_tensor)."""
        i = self.tensor_names().index(name)
        dims = [C.c_int() for _ in range(4)]
        _lib.check(self.lib.drs_vgg_tensor_shape(self.handle, i, *[C.byref(d) for d in dims]), "drs_vgg_tensor_shape")
        dst = torch.empty([d.value for d in dims], dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.drs_vgg_read_tensor(self.handle, i, C.c_void_p(self.workspace.data_ptr()),
                                                    C.c_void_p(dst.data_ptr()), _stream(self.device)), "drs_vgg_read_tensor")
        return dst

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            self.lib.drs_vgg_plan_destroy(h)
            self.handle = None


class _VGGLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, plan, pred, target):
        loss = plan.forward(pred, target, save=True)
        ctx.plan, ctx.generation = plan, plan.generation
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        plan = ctx.plan
        if plan.generation != ctx.generation:
            raise RuntimeError("VGGPerceptualLoss: another forward of the same shape ran between this loss and its backward; "
                               "its saved activations are gone")
        dpred = torch.empty((plan.B, 3, plan.H, plan.W), dtype=torch.float32, device=plan.device)
        plan.backward(grad_loss.detach().float().contiguous(), dpred)
        return None, dpred, None


class VGGPerceptualLoss(nn.Module):
    """Reference VGGPerceptualLoss(device) (:25-68) on the HIP path; `state_dict` replaces the torchvision checkpoint."""

    def __init__(self, device, state_dict=None):
        super().__init__()
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"VGGPerceptualLoss runs on a ROCm device, got {self.device} (no CPU path)")
        _lib.load()
        self._params = [t.to(self.device) for wb in feature_weights(state_dict) for t in wb]  # frozen: never updated
        self._plans = OrderedDict()

    def _plan(self, B, H, W):
        key = (B, H, W, vgg_impl())
        plan = self._plans.get(key)
        if plan is None:
            plan = _Plan(_lib.load(), self._params, B, H, W, key[3], self.device)
            plan.B, plan.H, plan.W = B, H, W
            self._plans[key] = plan
            while len(self._plans) > _MAX_PLANS:
                self._plans.popitem(last=False)
        else:
            self._plans.move_to_end(key)
        return plan

    def forward(self, x, y):
        if x.dim() != 4 or x.shape != y.shape:
            raise RuntimeError(f"VGGPerceptualLoss: inputs must be two (N, 3, H, W) tensors of one shape, got "
                               f"{tuple(x.shape)} and {tuple(y.shape)}")
        if x.shape[1] != 3:
            # the reference's in-place Normalize with 3 ImageNet channels raises on any other channel count (:42-51)
            raise RuntimeError(f"VGGPerceptualLoss needs 3-channel images (ImageNet mean/std over 3 channels), got "
                               f"{x.shape[1]} channels")
        if y.requires_grad:
            raise NotImplementedError("VGGPerceptualLoss: the target must not require a gradient (the training loss compares "
                                      "the predicted noise with the true noise)")
        for name, t in (("prediction", x), ("target", y)):
            if not t.is_cuda or t.dtype != torch.float32:
                raise RuntimeError(f"VGGPerceptualLoss: the {name} must be an fp32 ROCm tensor, got {t.dtype} on {t.device}")
        B, _, H, W = x.shape
        plan = self._plan(B, H, W)
        x, y = x.contiguous(), y.detach().contiguous()
        if torch.is_grad_enabled() and x.requires_grad:
            return _VGGLoss.apply(plan, x, y)
        return plan.forward(x.detach(), y, save=False)


class CombinedLoss(nn.Module):
    """Reference CombinedLoss (:65-77): weight_first * first(p, t) + (1 - weight_first) * second(p, t)."""

    def __init__(self, first_loss, second_loss, weight_first=0.5):
        super().__init__()
        self.first_loss = first_loss
        self.second_loss = second_loss
        self.weight_first = weight_first

    def forward(self, predicted, target):
        first_loss_value = self.first_loss(predicted, target)
        second_loss_value = self.second_loss(predicted, target)
        return self.weight_first * first_loss_value + (1 - self.weight_first) * second_loss_value


def mse_perceptual_noise(device, state_dict=None):
    """The loss `--loss MSE+Perceptual_noise` selects (reference :353-356)."""
    return CombinedLoss(first_loss=nn.MSELoss(), second_loss=VGGPerceptualLoss(device, state_dict), weight_first=0.3)
