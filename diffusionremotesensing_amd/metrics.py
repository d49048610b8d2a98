"""Image quality of a super-resolved batch `sr` against its ground truth `hr`: PSNR, SSIM, the spectral angle mapper (SAM)
and ERGAS, per image, computed where the samples live.

The sums over pixels come from two HIP kernels (csrc/metrics.hip through `hip_ops.metrics_pointwise` / `hip_ops.ssim_mean`);
what is left - a few float64 elements per image - is finalised with torch on the device.  Inputs are (B, C, H, W) fp32
ROCm tensors with 1 <= C <= 16 (a CPU tensor raises: there is no CPU path); `clamp=True` clamps both to [0, 1] first, as
the reference does before it shows a sample.  Every function returns a (B,) float64 device tensor.

    PSNR   10 log10(1 / MSE) over C, H, W (data range 1); inf for identical images
    SSIM   Wang et al. 2004: 11 x 11 Gaussian window (sigma 1.5), K1 = 0.01, K2 = 0.03, valid positions, mean over bands
    SAM    mean over pixels of the angle between the C-vectors of sr and hr, in degrees; pixels whose vector is exactly zero
           in either image are left out, an image without any other pixel gives NaN
    ERGAS  100 / magnification * sqrt(mean over bands of MSE_c / mean(hr_c)^2); a band whose hr mean is 0 makes it inf

`nodata=` (True or "nan": a pixel of hr with a NaN band; a number: also a pixel of hr whose bands all equal it) scores the
valid pixels of hr alone: PSNR over C nv elements, ERGAS' means over the nv valid pixels, SAM without the no-data pixels, SSIM
over the window positions whose 11 x 11 pixels are all valid (NaN when there is none); an image without a valid pixel gives
NaN in all four.  None is the unmasked path.
"""
import math

import torch

from . import hip_ops


def _psnr(sums, C, hw):
    return 10.0 * torch.log10(1.0 / (sums[:, :C].sum(dim=1) / (C * hw)))


def _sam(sums, C):
    return torch.rad2deg(sums[:, 2 * C] / sums[:, 2 * C + 1])  # 0 / 0: no pixel with an angle -> NaN


def _ergas(sums, C, hw, magnification_factor):
    mse, mean = sums[:, :C] / hw, sums[:, C:2 * C] / hw
    ratio = torch.where(mean == 0, torch.full_like(mse, math.inf), mse / (mean * mean))
    return 100.0 / magnification_factor * torch.sqrt(ratio.mean(dim=1))


def _need_bands(sr):
    if sr.dim() == 4 and sr.shape[1] < 2:
        raise ValueError(f"sam: the spectral angle needs at least 2 bands, got {sr.shape[1]}")


def _masked(sr, hr, nodata, clamp):
    """(sums (B, 2 C + 2), nv (B,)) of the pointwise launch over the valid pixels of hr."""
    out = hip_ops.metrics_pointwise_nodata(sr, hr, nodata, clamp)
    return out[:, :-1], out[:, -1]


def psnr(sr, hr, clamp=True, nodata=None):
    if nodata is not None:
        sums, nv = _masked(sr, hr, nodata, clamp)
        return _psnr(sums, sr.shape[1], nv)
    sums = hip_ops.metrics_pointwise(sr, hr, clamp)
    return _psnr(sums, sr.shape[1], sr.shape[2] * sr.shape[3])


def ssim(sr, hr, clamp=True, nodata=None):
    if nodata is not None:
        return hip_ops.ssim_nodata(sr, hr, nodata, clamp)[:, 0]
    return hip_ops.ssim_mean(sr, hr, clamp)


def sam(sr, hr, clamp=True, nodata=None):
    _need_bands(sr)
    if nodata is not None:
        return _sam(_masked(sr, hr, nodata, clamp)[0], sr.shape[1])
    return _sam(hip_ops.metrics_pointwise(sr, hr, clamp), sr.shape[1])


def ergas(sr, hr, magnification_factor, clamp=True, nodata=None):
    if nodata is not None:
        sums, nv = _masked(sr, hr, nodata, clamp)
        return _ergas(sums, sr.shape[1], nv[:, None], magnification_factor)
    sums = hip_ops.metrics_pointwise(sr, hr, clamp)
    return _ergas(sums, sr.shape[1], sr.shape[2] * sr.shape[3], magnification_factor)


def psnr_masked(sr, hr, where, clamp=True):
    """PSNR over the pixels selected by `where` alone ((B, 1 | C, H, W), nonzero = counted; a single-band selection counts the
    pixel in every band): the score of the filled-in region of a sample with known pixels.  A few torch operations in
    float64 on the device; an image with no selected pixel gives NaN."""
    a, b = (t.double().clamp(0, 1) if clamp else t.double() for t in (sr, hr))
    w = (where != 0).expand_as(a).double()
    mse = ((a - b) ** 2 * w).sum(dim=(1, 2, 3)) / w.sum(dim=(1, 2, 3))
    return 10.0 * torch.log10(1.0 / mse)


def image_quality(sr, hr, magnification_factor=None, clamp=True, nodata=None):
    """{"psnr", "ssim"[, "sam" when C >= 2][, "ergas" when a magnification is given]}: the values of the single functions,
    from one pointwise launch and one SSIM launch.  With `nodata` also "valid_fraction", the share of hr's pixels that are
    data."""
    C, hw = sr.shape[1], sr.shape[2] * sr.shape[3]
    if nodata is not None:
        sums, nv = _masked(sr, hr, nodata, clamp)
        out = {"psnr": _psnr(sums, C, nv), "ssim": hip_ops.ssim_nodata(sr, hr, nodata, clamp)[:, 0]}
        if C >= 2:
            out["sam"] = _sam(sums, C)
        if magnification_factor is not None:
            out["ergas"] = _ergas(sums, C, nv[:, None], magnification_factor)
        out["valid_fraction"] = nv / hw
        return out
    sums = hip_ops.metrics_pointwise(sr, hr, clamp)
    out = {"psnr": _psnr(sums, C, hw), "ssim": hip_ops.ssim_mean(sr, hr, clamp)}
    if C >= 2:
        out["sam"] = _sam(sums, C)
    if magnification_factor is not None:
        out["ergas"] = _ergas(sums, C, hw, magnification_factor)
    return out
