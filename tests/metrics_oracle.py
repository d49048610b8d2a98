"""Float64 restatement of diffusionremotesensing_amd.metrics, written from the definitions (test oracle).

sr, hr: (B, C, H, W) tensors of any float dtype; every function returns a (B,) float64 tensor.
"""
import math

import torch
import torch.nn.functional as F


def _prep(sr, hr, clamp):
    sr, hr = sr.detach().cpu().double(), hr.detach().cpu().double()
    if clamp:
        sr, hr = sr.clamp(0, 1), hr.clamp(0, 1)
    return sr, hr


def psnr(sr, hr, clamp=True):
    sr, hr = _prep(sr, hr, clamp)
    mse = ((sr - hr) ** 2).mean(dim=(1, 2, 3))
    return 10.0 * torch.log10(1.0 / mse)


def gaussian_window(size=11, sigma=1.5):
    k = torch.arange(size, dtype=torch.float64) - size // 2
    g = torch.exp(-k * k / (2.0 * sigma * sigma))
    g = g / g.sum()
    return g[:, None] * g[None, :]


def ssim(sr, hr, clamp=True):
    """Wang et al. 2004: 11 x 11 Gaussian window (sigma 1.5), K1 = 0.01, K2 = 0.03, data range 1, valid positions only,
    per band, mean over positions and bands."""
    sr, hr = _prep(sr, hr, clamp)
    B, C, H, W = sr.shape
    w = gaussian_window()[None, None]

    def blur(t):
        return F.conv2d(t.reshape(B * C, 1, H, W), w).reshape(B, C, H - 10, W - 10)
    mx, my = blur(sr), blur(hr)
    vx, vy, cxy = blur(sr * sr) - mx * mx, blur(hr * hr) - my * my, blur(sr * hr) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return s.mean(dim=(1, 2, 3))


def sam(sr, hr, clamp=True):
    """Mean over pixels of the angle between the C-vectors, in degrees, as 2 atan2(|u^ - v^|, |u^ + v^|) on the normalised
    vectors; a pixel whose vector is exactly zero in either image is left out (no such pixel left: NaN)."""
    sr, hr = _prep(sr, hr, clamp)
    nu, nv = sr.norm(dim=1, keepdim=True), hr.norm(dim=1, keepdim=True)
    valid = ((nu != 0) & (nv != 0))[:, 0]
    u, v = sr / nu, hr / nv
    ang = 2.0 * torch.atan2((u - v).norm(dim=1), (u + v).norm(dim=1))
    ang = torch.where(valid, ang, torch.zeros_like(ang))
    return torch.rad2deg(ang.sum(dim=(1, 2)) / valid.sum(dim=(1, 2)))


def ergas(sr, hr, magnification_factor, clamp=True):
    """100 / magnification * sqrt(mean over bands of MSE_c / mean(hr_c)^2); a band whose hr mean is 0 makes it inf."""
    sr, hr = _prep(sr, hr, clamp)
    mse = ((sr - hr) ** 2).mean(dim=(2, 3))
    mean = hr.mean(dim=(2, 3))
    ratio = torch.where(mean == 0, torch.full_like(mse, math.inf), mse / (mean * mean))
    return 100.0 / magnification_factor * torch.sqrt(ratio.mean(dim=1))


def image_quality(sr, hr, magnification_factor=None, clamp=True):
    out = {"psnr": psnr(sr, hr, clamp), "ssim": ssim(sr, hr, clamp)}
    if sr.shape[1] >= 2:
        out["sam"] = sam(sr, hr, clamp)
    if magnification_factor is not None:
        out["ergas"] = ergas(sr, hr, magnification_factor, clamp)
    return out
