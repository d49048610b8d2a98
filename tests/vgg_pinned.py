"""Float64 references of the VGG19 loss (csrc/vgg_loss.hip) that take every discrete choice from the run under test.

The loss is piecewise linear in its ReLU masks and max-pool winners; a float64 oracle run from the image decides a few near
ties otherwise than any fp32 run, and those flips alone move d(loss)/d(pred) by 1e-3 .. 1.5e-2.  The
references here are "pinned" to the run they judge:

  forward_layers    every layer is relu(conv2d) in float64 of the run's OWN previous tensor (max-pooled where a pool follows),
                    so a layer's error does not compound and no flip matters;
  pinned_backward   the float64 backward whose ReLU masks and pool winners are read from the run's saved activations and
                    whose seed comes from the run's features: what is left is the linear arithmetic of the backward.

`Steps` holds the backward's operations one by one; the host tests subclass it to break a single step (mutations).
"""
import torch
import torch.nn.functional as F

import vgg_oracle as O
from diffusionremotesensing_amd.perceptual import FEATURE_CONVS

F64 = torch.float64


def weight(sd, l):
    return sd[f"features.{FEATURE_CONVS[l]}.weight"].to(F64)


def bias(sd, l):
    return sd[f"features.{FEATURE_CONVS[l]}.bias"].to(F64)


def prep_reference(img):
    """float64 F.interpolate(bicubic, align_corners=False) to 224 x 224 when the width is not 224, then Normalize."""
    return O.preprocess(img.to(F64))


def forward_layers(sd, x0_dev, saved_dev):
    """[relu(conv2d_f64(input of layer l))] for l = 0 .. 15.  x0_dev: the run's (N, 3, H0, W0) prep output; saved_dev: its 16
    ReLU outputs.  The input of layer l > 0 is saved_dev[l - 1], max-pooled exactly where a pool follows layer l - 1."""
    out = []
    x = x0_dev.to(F64)
    for l in range(len(FEATURE_CONVS)):
        out.append(F.relu(F.conv2d(x, weight(sd, l), bias(sd, l), padding=1)))
        x = saved_dev[l].to(F64)
        if l in O.POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return out


def pool_winners(y):
    """(N, C, OH, OW) index 0 .. 3 (= 2 dy + dx) of the first maximum of each 2 x 2 window of y, in window order."""
    N, C, H, W = y.shape
    OH, OW = H // 2, W // 2
    win = y[:, :, :2 * OH, :2 * OW].reshape(N, C, OH, 2, OW, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, OH, OW, 4)
    return win.argmax(-1)  # torch documents the first maximal index


def scatter_windows(vals, H, W):
    """(N, C, OH, OW, 4) values per window slot -> (N, C, H, W), zeros in the row / column the floor drops."""
    N, C, OH, OW, _ = vals.shape
    out = vals.new_zeros((N, C, H, W))
    out[:, :, :2 * OH, :2 * OW] = vals.reshape(N, C, OH, OW, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * OH, 2 * OW)
    return out


class Steps:
    """The backward, one operation per method (l = 0-based conv index)."""

    def seed(self, fx, fy, grad_loss):
        return 2.0 * (fx - fy) / fx.numel() * grad_loss

    def pool_adjoint(self, l, g, y):
        """Gradient of MaxPool2d(2, 2) after layer l: all of it to the first maximum of the saved values y."""
        onehot = F.one_hot(pool_winners(y), 4).to(g.dtype)
        return scatter_windows(onehot * g[..., None], y.shape[-2], y.shape[-1])

    def relu_mask(self, l, g, y):
        return g * (y > 0)

    def conv_dgrad(self, l, g, w):
        return F.conv_transpose2d(g, w, padding=1)

    def resize_adjoint(self, g, H, W):
        return O.resize_adjoint_by_taps(g, H, W)


def pinned_backward(sd, saved_dev, features_dev, grad_loss, in_hw, steps=None, stop_at=0):
    """float64 d(grad_loss * loss)/d(pred), (B, 3, H, W), pinned to one run: saved_dev = its 16 prediction-half ReLU outputs,
    features_dev = its (2B, 512, h5, w5) features, in_hw = (H, W) of the images.  stop_at = l > 0 returns instead the
    gradient w.r.t. the input of layer l (to bisect a failure)."""
    steps = steps or Steps()
    B = features_dev.shape[0] // 2
    f = features_dev.to(F64)
    g = steps.seed(f[:B], f[B:], float(grad_loss))
    for l in reversed(range(stop_at, len(FEATURE_CONVS))):
        y = saved_dev[l]
        if l in O.POOL_AFTER:
            g = steps.pool_adjoint(l, g, y)
        g = steps.relu_mask(l, g, y)
        g = steps.conv_dgrad(l, g, weight(sd, l))
    if stop_at:
        return g
    g = g / torch.tensor(O.STD, dtype=F64).view(-1, 1, 1)
    H, W = in_hw
    return steps.resize_adjoint(g, H, W) if W != 224 else g


def run_torch(sd, x, y, dtype, grad_loss=1.0):
    """The loss in plain torch at `dtype` with autograd: (x0, saved, features, loss, dpred), the tensors a device run hands
    out (x0: (2B, 3, H0, W0); saved: the prediction half's ReLU outputs; features: (2B, 512, h5, w5)).  The resize goes
    through the kernel's tap tables (vgg_oracle.resize_by_taps: built in double, rounded to `dtype`) - ATen's own fp32
    bicubic computes the source coordinate in fp32 (an ulp of 3e-5 at 300 rows, passed on to the tap weights): 1.8e-5 in
    dpred at 300 x 260, against 6e-7 with the tables."""
    B = x.shape[0]
    xr = x.detach().to(dtype).requires_grad_(True)
    t = torch.cat([xr, y.detach().to(dtype)])
    if t.shape[-1] != 224:
        t = O.resize_by_taps(t, 224, 224)
    t = O.preprocess(t)
    x0 = t.detach()
    saved = []
    for l, k in enumerate(FEATURE_CONVS):
        t = F.relu(F.conv2d(t, sd[f"features.{k}.weight"].to(dtype), sd[f"features.{k}.bias"].to(dtype), padding=1))
        saved.append(t.detach()[:B])
        if l in O.POOL_AFTER:
            t = F.max_pool2d(t, 2, 2)
    loss = torch.mean((t[:B] - t[B:]) ** 2)
    (grad_loss * loss).backward()
    return x0, saved, t.detach(), loss.item(), xr.grad.detach()
