"""Float64 restatement of the reference's perceptual loss (train_diffusion_superres.py:25-77) in torch.functional.

  P(img)   = Normalize(ImageNet)(F.interpolate(img, (224, 224), 'bicubic', align_corners=False) if width != 224 else img)
  F(x)     = vgg19().features: 16 x (conv3x3 p1 + ReLU), MaxPool2d(2, 2) after convs 2, 4, 8, 12, 16
  vgg      = mean((F(P(x)) - F(P(y)))**2);  combined = 0.3 * mse + 0.7 * vgg

Also the bicubic tap tables of csrc/vgg_loss.hip (ATen's upsample_bicubic2d as 4 taps per output row / column) and their
transpose, so that the CPU tests can hold the kernel's indexing against F.interpolate.
"""
import math

import torch
import torch.nn.functional as F

from diffusionremotesensing_amd.perceptual import FEATURE_CHANNELS, FEATURE_CONVS

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
POOL_AFTER = (1, 3, 7, 11, 15)  # conv indices (0-based) a max-pool follows


def seeded_vgg_state_dict(seed=0, classifier=False):
    """vgg19 state dict with torchvision's key layout and seeded weights: He scale std = sqrt(2 / (9 Cin)) (activations keep
    their size across 16 layers) and small biases.  classifier=True adds stand-in `classifier.*` entries."""
    from diffusionremotesensing_amd import synthetic
    sd = {}
    cin = 3
    for k, cout in zip(FEATURE_CONVS, FEATURE_CHANNELS):
        sd[f"features.{k}.weight"] = synthetic.tensor_normal(f"vgg.features.{k}.weight", (cout, cin, 3, 3), seed,
                                                             std=math.sqrt(2.0 / (9 * cin)))
        sd[f"features.{k}.bias"] = synthetic.tensor_normal(f"vgg.features.{k}.bias", (cout,), seed, std=0.05)
        cin = cout
    if classifier:
        for i, shape in ((0, (16, 25088)), (3, (16, 16)), (6, (10, 16))):
            sd[f"classifier.{i}.weight"] = synthetic.tensor_normal(f"vgg.classifier.{i}.weight", shape, seed, std=0.01)
            sd[f"classifier.{i}.bias"] = torch.zeros(shape[0])
    return sd


def preprocess(img):
    if img.shape[-1] != 224:  # the reference tests the width only
        img = F.interpolate(img, size=(224, 224), mode="bicubic", align_corners=False)
    if img.shape[-3] != 3:
        raise RuntimeError(f"Normalize with 3 channel statistics on a {img.shape[-3]}-channel image")
    mean = torch.tensor(MEAN, dtype=img.dtype).view(-1, 1, 1)
    std = torch.tensor(STD, dtype=img.dtype).view(-1, 1, 1)
    return (img - mean) / std


def features(sd, x):
    for l, k in enumerate(FEATURE_CONVS):
        x = F.relu(F.conv2d(x, sd[f"features.{k}.weight"].to(x.dtype), sd[f"features.{k}.bias"].to(x.dtype), padding=1))
        if l in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return x


def vgg_loss(sd, x, y):
    return torch.mean((features(sd, preprocess(x)) - features(sd, preprocess(y))) ** 2)


def combined_loss(sd, pred, noise, weight_first=0.3):
    return weight_first * F.mse_loss(pred, noise) + (1 - weight_first) * vgg_loss(sd, pred, noise)


def vgg_loss_and_grad(sd, x, y, dtype=torch.float64):
    """(loss, d loss / d x) in `dtype`."""
    x = x.detach().to(dtype).requires_grad_(True)
    loss = vgg_loss(sd, x, y.detach().to(dtype))
    loss.backward()
    return loss.item(), x.grad.detach()


# ---- the kernel's resampling tables ------------------------------------------------------------------------------------
def _cubic1(x, A):
    return ((A + 2) * x - (A + 3)) * x * x + 1


def _cubic2(x, A):
    return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A


def bicubic_taps(n_in, n_out):
    """(idx, w): (n_out, 4) source indices and weights of one axis, as bicubic_taps() in csrc/vgg_loss.hip builds them:
    src = scale * (dst + 0.5) - 0.5 with scale = n_in / n_out and no clamping, taps floor(src) - 1 .. + 2 clamped to the
    image, cubic convolution weights with A = -0.75."""
    A, scale = -0.75, n_in / n_out
    idx = torch.empty((n_out, 4), dtype=torch.long)
    w = torch.empty((n_out, 4), dtype=torch.float64)
    for o in range(n_out):
        src = scale * (o + 0.5) - 0.5
        f = math.floor(src)
        t = src - f
        for k, c in enumerate((_cubic2(t + 1, A), _cubic1(t, A), _cubic1(1 - t, A), _cubic2(2 - t, A))):
            idx[o, k] = min(max(f - 1 + k, 0), n_in - 1)
            w[o, k] = c
    return idx, w


def resize_by_taps(img, out_h, out_w):
    """The prep kernel's resize: per output pixel, 4 rows interpolated along x, then the 4 row values along y."""
    iy, wy = bicubic_taps(img.shape[-2], out_h)
    ix, wx = bicubic_taps(img.shape[-1], out_w)
    rows = (img[..., ix] * wx.to(img.dtype)).sum(-1)                    # (..., H, out_w, )
    return (rows[..., iy, :] * wy.to(img.dtype)[:, :, None]).sum(-2)    # (..., out_h, out_w)


def resize_adjoint_by_taps(g, n_h, n_w):
    """The backward kernels' bicubic adjoint: per input index, a gather over the transpose of the tap table (x, then y)."""
    iy, wy = bicubic_taps(n_h, g.shape[-2])
    ix, wx = bicubic_taps(n_w, g.shape[-1])
    mx = torch.zeros((g.shape[-1], n_w), dtype=g.dtype)
    mx.index_put_((torch.arange(g.shape[-1])[:, None].expand(-1, 4), ix), wx.to(g.dtype), accumulate=True)
    my = torch.zeros((g.shape[-2], n_h), dtype=g.dtype)
    my.index_put_((torch.arange(g.shape[-2])[:, None].expand(-1, 4), iy), wy.to(g.dtype), accumulate=True)
    return my.t() @ (g @ mx)
