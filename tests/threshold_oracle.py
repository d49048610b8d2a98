"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of dynamic thresholding as `Diffusion(x0_clip=, x0_threshold=)` defines it (Saharia et
al., "Imagen", 2022, section 2.3), written from the definition and not from the kernel: per image, x0 = the clean image the
prediction implies (`prediction_oracle.to_x0`), d = x0 - c with c = (lo + hi) / 2 and r = (hi - lo) / 2 rounded to fp32 as the
library forms them, s = the (k + 1)-th smallest |d| (torch.kthvalue; a NaN or an infinity ranks as +inf), k = floor(p (chw - 1)).
Where s <= r or s is not finite the image takes the static clamp; otherwise x0 becomes clamp(c + clamp(d, -s, s) r / s, lo, hi).
A non-finite element stays what it is.  eps = (x_t - a x0) / s as `prediction_oracle.to_eps`.
"""
import math

import numpy as np
import torch

import prediction_oracle as PO


def rank_of(p, chw):
    """k = floor(p (chw - 1)), the 0-based rank of torch.quantile(..., interpolation="lower")."""
    return int(math.floor(p * (chw - 1)))


def centre_and_half_range(clip):
    lo, hi = clip
    return float(np.float32((float(lo) + float(hi)) / 2.0)), float(np.float32((float(hi) - float(lo)) / 2.0))


def scales_of(x0, clip, p):
    """(n,) float64: per image the rank-k value of |x0 - c|, non-finite values ranked as +inf; x0 float64 (n, ...)."""
    c, _ = centre_and_half_range(clip)
    dev = (x0.double() - c).abs().flatten(1)
    dev = torch.where(torch.isfinite(dev), dev, torch.full_like(dev, math.inf))
    return dev.kthvalue(rank_of(p, dev.shape[1]) + 1, dim=1).values


def threshold_x0(x0, clip, p):
    """(thresholded x0, scales) of float64 x0 (n, C, H, W)."""
    lo, hi = clip
    c, r = centre_and_half_range(clip)
    x0 = x0.double()
    s = scales_of(x0, clip, p)
    sv = s.view(-1, 1, 1, 1)
    dynamic = (sv > r) & torch.isfinite(sv)
    safe = torch.where(dynamic, sv, torch.ones_like(sv))
    d = x0 - c
    q_dyn = (c + torch.minimum(torch.maximum(d, -safe), safe) * (r / safe)).clamp(lo, hi)
    q = torch.where(dynamic, q_dyn, x0.clamp(lo, hi))
    return torch.where(torch.isfinite(x0), q, x0), s


def to_eps(kind, pred, x_t, alpha_hat, t, clip, p):
    """(eps, bound, scales): the noise the thresholded x0 implies, the sum of the absolute terms of its expression per element
    (`prediction_oracle._over_s`: the scale an fp32 evaluation's rounding is measured against) and the n scales.  Where s == 0
    (alpha_hat == 1) there is no noise to name: eps 0, and the library reports the scale 0 there."""
    a, s = PO.a_s(alpha_hat, t)
    if kind == "eps" and bool((a == 0).any()):
        raise NotImplementedError("a == 0 (zero terminal SNR): an eps prediction is passed through; not tabulated here")
    x0 = PO.to_x0(kind, pred, x_t, alpha_hat, t)
    q, scales = threshold_x0(x0, clip, p)
    live = (s != 0).reshape(-1)
    scales = torch.where(live.expand_as(scales), scales, torch.zeros_like(scales))
    eps, bound = PO._over_s(x_t.double(), a * q, s)
    return eps, bound, scales


def eps_fn_of(kind, clip, p, alpha_hat, pred_fn):
    """eps_fn(x_fp32, t) for the float64 chains (ddim_oracle, dpm_oracle, inpaint_oracle, prediction_oracle.chain's ancestral
    loop) from pred_fn(x_fp32, t) -> the model's output, as `prediction_oracle.eps_fn_of` with the threshold in place of the clip."""
    def eps_fn(x, t):
        return to_eps(kind, pred_fn(x, t), x, alpha_hat, t, clip, p)[0]
    return eps_fn


def chain(kind, clip, p, pred_fn, shape, noise_steps, schedule, sampler, noise_source):
    """`prediction_oracle.chain` with the thresholded eps."""
    import ddim_oracle as O
    import dpm_oracle as P
    from oracle import diffusion_oracle as D
    alpha, alpha_hat, beta = schedule
    eps_fn = eps_fn_of(kind, clip, p, alpha_hat, pred_fn)
    if sampler[0] == "ddim":
        return O.chain(eps_fn, shape, noise_steps, alpha_hat, sampler[1], sampler[2], noise_source)
    if sampler[0] == "dpmpp_2m":
        return P.chain(eps_fn, shape, noise_steps, alpha_hat, sampler[1], noise_source)
    n = shape[0]
    x = noise_source(noise_steps, shape).double()
    a64, ah64, b64 = alpha.double(), alpha_hat.double(), beta.double()
    for i in reversed(range(1, noise_steps)):
        eps = eps_fn(x.float(), i)
        z = noise_source(i, shape).double() if i > 1 else torch.zeros_like(x)
        x = D.sampler_step(x, eps, z, torch.full((n,), i, dtype=torch.long), a64, ah64, b64)
    return x
