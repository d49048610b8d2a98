"""Float64 restatement of the four no-data entry points (include/drs_hip.h: drs_noise_target_nodata,
drs_diffusion_loss_masked, drs_metrics_pointwise_nodata, drs_ssim_nodata), written from their definitions (test oracle).

One rule everywhere: a pixel of a clean / truth image (..., C, H, W) is no-data when any of its bands is NaN, or when a finite
`nodata_value` is given and all of its bands equal it as fp32.  Everything a masked sum leaves out is removed by selection
(torch.where / boolean indexing), never by a product with zero, so that a NaN or an infinity under the mask cannot reach a
result here either."""
import math

import torch

import loss_oracle as LO
import metrics_oracle as MO


def valid_mask(x, nodata_value=None):
    """(..., H, W) bool, True = data, of an fp32 image (..., C, H, W); nodata_value None or NaN: the NaN rule alone."""
    assert x.dtype == torch.float32
    nodata = torch.isnan(x).any(dim=-3)
    if nodata_value is not None and not math.isnan(float(nodata_value)):
        assert math.isfinite(float(nodata_value))
        nodata = nodata | (x == torch.tensor(float(nodata_value), dtype=torch.float32)).all(dim=-3)
    return ~nodata


def noise_target(x0, eps, t, alpha_hat, prediction, nodata_value=None, fill=0.5):
    """(x_t, target, valid) in float64 (valid: (n, H, W) bool).  a = sqrt(alpha_hat[t]) and b = sqrt(1 - alpha_hat[t]) are the
    kernel's fp32 values (widened); products and sums are exact-then-float64, so a valid element differs from the kernel's by
    the fp32 roundings of two products and one sum.  A t outside the table: NaN, and no valid pixel."""
    n = x0.shape[0]
    valid = valid_mask(x0, nodata_value)
    ok_t = (t >= 0) & (t < alpha_hat.numel())
    ah = alpha_hat.float()[t.clamp(0, alpha_hat.numel() - 1)]
    a, b = torch.sqrt(ah).double().view(n, 1, 1, 1), torch.sqrt(1.0 - ah).double().view(n, 1, 1, 1)
    x, e = x0.double(), eps.double()
    m = valid[:, None].expand_as(x)
    x_in = torch.where(m, x, torch.full_like(x, float(fill)))
    x_t = a * x_in + b * e
    target = {"eps": e, "v": a * e - b * x, "x0": x}[prediction]
    target = torch.where(m, target, torch.zeros_like(x))
    bad = ~ok_t.view(n, 1, 1, 1)
    nan = torch.full_like(x, math.nan)
    return torch.where(bad, nan, x_t), torch.where(bad, nan, target), valid & ok_t.view(n, 1, 1)


def masked_loss(pred, target, valid, kind, delta=1.0, w=None):
    """(per_image (B,), loss (), grad of pred's shape, counts (B,) int64, Bv), float64, for fp32 pred / target (B, C, H, W) and
    valid (B, H, W) bool:  per_image[b] = (1 / n_b) sum over valid elements of l(d), 0 when nv_b = 0;  loss = (1 / Bv) sum over
    nv_b > 0 of w_b per_image[b], 0 when Bv = 0;  grad = w_b / (Bv n_b) l'(d) at valid elements, 0 elsewhere."""
    assert pred.dtype == torch.float32 and target.dtype == torch.float32 and valid.dtype == torch.bool
    B, C = pred.shape[:2]
    m = valid[:, None].expand_as(pred)
    zero = torch.zeros_like(pred)
    d = (torch.where(m, pred, zero) - torch.where(m, target, zero)).double()  # the fp32 difference of the selected values
    l, lp = LO.element_loss(d, kind, delta)
    l, lp = torch.where(m, l, torch.zeros_like(l)), torch.where(m, lp, torch.zeros_like(lp))
    counts = valid.reshape(B, -1).sum(dim=1)
    n_b = (C * counts).double()
    has = counts > 0
    Bv = int(has.sum())
    per_image = torch.where(has, l.reshape(B, -1).sum(dim=1) / n_b.clamp_min(1.0), torch.zeros(B, dtype=torch.float64))
    w = torch.ones(B, dtype=torch.float64) if w is None else w
    loss = torch.where(has, w * per_image, torch.zeros(B, dtype=torch.float64)).sum() / Bv if Bv else torch.zeros((), dtype=torch.float64)
    coef = torch.where(has, w / (max(Bv, 1) * n_b.clamp_min(1.0)), torch.zeros(B, dtype=torch.float64))
    grad = torch.where(m, coef.view(B, 1, 1, 1) * lp, torch.zeros_like(lp))
    return per_image, loss, grad, counts, Bv


def pointwise_sums(sr, hr, nodata_value=None, clamp=True):
    """(B, 2 C + 3) float64: per band the squared error and the sum of hr, the sum of the per-pixel angles (radians), the number
    of pixels in that sum and the number of valid pixels - all over the valid pixels of hr (the mask before the clamp)."""
    valid = valid_mask(hr, nodata_value)
    B, C = sr.shape[:2]
    m = valid[:, None].expand_as(sr)
    zero = torch.zeros_like(sr)
    s, h = MO._prep(torch.where(m, sr, zero), torch.where(m, hr, zero), clamp)
    sse = torch.where(m, (s - h) ** 2, torch.zeros_like(s)).sum(dim=(2, 3))
    shr = torch.where(m, h, torch.zeros_like(h)).sum(dim=(2, 3))
    nu, nv = s.norm(dim=1, keepdim=True), h.norm(dim=1, keepdim=True)
    has = valid & ((nu != 0) & (nv != 0))[:, 0]
    ones = torch.ones_like(nu)
    u, v = s / torch.where(nu == 0, ones, nu), h / torch.where(nv == 0, ones, nv)
    ang = 2.0 * torch.atan2((u - v).norm(dim=1), (u + v).norm(dim=1))
    ang = torch.where(has, ang, torch.zeros_like(ang)).sum(dim=(1, 2))
    return torch.cat([sse, shr, ang[:, None], has.sum(dim=(1, 2)).double()[:, None], valid.sum(dim=(1, 2)).double()[:, None]], dim=1)


def ssim(sr, hr, nodata_value=None, clamp=True):
    """(B, 2) float64: the mean SSIM over bands and over the window positions whose 11 x 11 pixels are all valid (NaN when there
    is none), and the number of those positions per band."""
    valid = valid_mask(hr, nodata_value)
    B, C, H, W = sr.shape
    m = valid[:, None].expand_as(sr)
    zero = torch.zeros_like(sr)
    s, h = MO._prep(torch.where(m, sr, zero), torch.where(m, hr, zero), clamp)
    w = MO.gaussian_window()[None, None]
    F = torch.nn.functional

    def blur(t):
        return F.conv2d(t.reshape(B * C, 1, H, W), w).reshape(B, C, H - 10, W - 10)
    mx, my = blur(s), blur(h)
    vx, vy, cxy = blur(s * s) - mx * mx, blur(h * h) - my * my, blur(s * h) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    q = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    full = F.conv2d(valid[:, None].double(), torch.ones(1, 1, 11, 11, dtype=torch.float64)) == 121.0  # (B, 1, H - 10, W - 10)
    n = full.sum(dim=(1, 2, 3)).double()
    total = torch.where(full.expand_as(q), q, torch.zeros_like(q)).sum(dim=(1, 2, 3))
    mean = torch.where(n > 0, total / (C * n.clamp_min(1.0)), torch.full_like(n, math.nan))
    return torch.stack([mean, n], dim=1)


def image_quality(sr, hr, magnification_factor=None, nodata_value=None, clamp=True):
    """metrics.image_quality(nodata=): PSNR over C nv elements, ERGAS' means over the nv valid pixels, SAM without the no-data
    pixels, SSIM as `ssim`, and valid_fraction = nv / (H W)."""
    C, hw = sr.shape[1], sr.shape[2] * sr.shape[3]
    sums = pointwise_sums(sr, hr, nodata_value, clamp)
    nv = sums[:, 2 * C + 2]
    out = {"psnr": 10.0 * torch.log10(1.0 / (sums[:, :C].sum(dim=1) / (C * nv))), "ssim": ssim(sr, hr, nodata_value, clamp)[:, 0]}
    if C >= 2:
        out["sam"] = torch.rad2deg(sums[:, 2 * C] / sums[:, 2 * C + 1])
    if magnification_factor is not None:
        mse, mean = sums[:, :C] / nv[:, None], sums[:, C:2 * C] / nv[:, None]
        ratio = torch.where(mean == 0, torch.full_like(mse, math.inf), mse / (mean * mean))
        out["ergas"] = 100.0 / magnification_factor * torch.sqrt(ratio.mean(dim=1))
    out["valid_fraction"] = nv / hw
    return out
