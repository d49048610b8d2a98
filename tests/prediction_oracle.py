"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of what `Diffusion(prediction=, x0_clip=)` adds: the three parameterisations of a
network's output - eps, v = a eps - s x0 (Salimans & Ho 2022) and x0, with a = sqrt(ah), s = sqrt(1 - ah) - converted into each
other, the training target, the Min-SNR weights of each, and wrappers that hand the existing float64 chains (ddim_oracle,
dpm_oracle, oracle.diffusion_oracle) an eps converted from the oracle UNet's output.  The coefficients are float64 functions of
the fp32 table entry, as the kernels read it.  Written from the definitions (x_t = a x0 + s eps), not from the kernel's forms.
"""
import math

import torch

import ddim_oracle as O
import dpm_oracle as P
from oracle import diffusion_oracle as D

KINDS = ("eps", "v", "x0")


def a_s(alpha_hat, t):
    """(a, s) per entry of t (an int or an int tensor), float64 from the fp32 table, shaped to broadcast over (n, C, H, W)."""
    ah = torch.as_tensor(alpha_hat)[torch.as_tensor(t)].double()
    a, s = torch.sqrt(ah), torch.sqrt(1.0 - ah)
    return (a.view(-1, 1, 1, 1), s.view(-1, 1, 1, 1)) if ah.dim() else (a, s)


def from_eps(kind, eps, x_t, alpha_hat, t):
    """What a perfect network of `kind` returns where the noise in x_t is eps: x0 = (x_t - s eps) / a, v = a eps - s x0."""
    a, s = a_s(alpha_hat, t)
    eps, x_t = eps.double(), x_t.double()
    if kind == "eps":
        return eps
    x0 = (x_t - s * eps) / a
    return x0 if kind == "x0" else a * eps - s * x0


def to_x0(kind, pred, x_t, alpha_hat, t):
    """The clean image a prediction implies: x0 = a x_t - s v = (x_t - s eps) / a."""
    a, s = a_s(alpha_hat, t)
    pred, x_t = pred.double(), x_t.double()
    return {"eps": lambda: (x_t - s * pred) / a, "v": lambda: a * x_t - s * pred, "x0": lambda: pred}[kind]()


def to_eps(kind, pred, x_t, alpha_hat, t, clip=None):
    """The noise a prediction implies, eps = (x_t - a x0) / s = s x_t + a v; with `clip` = (lo, hi) the implied x0 is clamped
    first (a NaN or an infinity stays what it is).  Returns (eps, bound): `bound` is the largest sum of the absolute terms of
    the expressions evaluated, per element - the scale an fp32 evaluation's rounding errors are measured against."""
    a, s = a_s(alpha_hat, t)
    pred, x_t = pred.double(), x_t.double()
    if clip is None:
        if kind == "eps":
            return pred, pred.abs()
        if kind == "v":
            return s * x_t + a * pred, (s * x_t).abs() + (a * pred).abs()
        return _over_s(x_t, a * pred, s)
    if kind == "eps" and bool((a == 0).any()):
        raise NotImplementedError("a == 0 (zero terminal SNR): an eps prediction is passed through unclipped; not tabulated here")
    x0 = to_x0(kind, pred, x_t, alpha_hat, t)
    x0c = torch.where(torch.isfinite(x0), x0.clamp(clip[0], clip[1]), x0)
    return _over_s(x_t, a * x0c, s)


def _over_s(x_t, a_x0, s):
    """((x_t - a x0) / s, |x_t / s| + |a x0 / s|); where s == 0 (alpha_hat == 1: there is no noise to name) both are 0."""
    live = (s != 0).expand_as(x_t)
    safe = torch.where(s != 0, s, torch.ones_like(s))
    zero = torch.zeros_like(x_t)
    return torch.where(live, (x_t - a_x0) / safe, zero), torch.where(live, (x_t / safe).abs() + (a_x0 / safe).abs(), zero)


def x0_terms(kind, pred, x_t, alpha_hat, t):
    """Sum of the absolute terms of `to_x0`'s expression (the rounding scale of the x0 a clip sees)."""
    a, s = a_s(alpha_hat, t)
    pred, x_t = pred.double(), x_t.double()
    return {"eps": lambda: (x_t / a).abs() + (s * pred / a).abs(), "v": lambda: (a * x_t).abs() + (s * pred).abs(),
            "x0": lambda: pred.abs()}[kind]()


def v_target(x0, eps, alpha_hat, t):
    """(x_t, v) = (a x0 + s eps, a eps - s x0) with a = sqrt(ah), s = sqrt(1 - ah) rounded to fp32 as the training kernels form
    them, products and sums in float64; also the sums of the absolute terms of both."""
    ah = torch.as_tensor(alpha_hat)[torch.as_tensor(t)].float()
    a, s = torch.sqrt(ah).double().view(-1, 1, 1, 1), torch.sqrt(1.0 - ah).double().view(-1, 1, 1, 1)
    x0, eps = x0.double(), eps.double()
    return a * x0 + s * eps, a * eps - s * x0, (a * x0).abs() + (s * eps).abs(), (a * eps).abs() + (s * x0).abs()


def target(kind, x0, eps, alpha_hat, t):
    """The regression target of a training step."""
    return {"eps": lambda: eps.double(), "x0": lambda: x0.double(), "v": lambda: v_target(x0, eps, alpha_hat, t)[1]}[kind]()


def weights(kind, alpha_hat, gamma):
    """Min-SNR-gamma weights (T,) float64: min(SNR, gamma) / SNR, / (SNR + 1), / 1; at SNR = inf: 0, 0, gamma."""
    out = []
    for ah in torch.as_tensor(alpha_hat).double().tolist():
        snr = math.inf if ah >= 1.0 else ah / (1.0 - ah)
        m = min(snr, gamma)
        out.append({"eps": 0.0 if math.isinf(snr) else (m / snr if snr > 0 else 1.0),
                    "v": 0.0 if math.isinf(snr) else m / (snr + 1.0), "x0": m}[kind])
    return torch.tensor(out, dtype=torch.float64)


# -- chains: the existing float64 chains on an eps converted from the model's output ----------------------------------------------
def eps_fn_of(kind, clip, alpha_hat, pred_fn):
    """eps_fn(x_fp32, t) for ddim_oracle.chain / dpm_oracle.chain from pred_fn(x_fp32, t) -> the model's output (any float
    dtype; a guided one already combined)."""
    def eps_fn(x, t):
        return to_eps(kind, pred_fn(x, t), x, alpha_hat, t, clip)[0]
    return eps_fn


def superres_pred_fn(model, n, lr_img, magnification_factor):
    lr = lr_img if lr_img.dim() == 4 else lr_img.unsqueeze(0)
    return lambda x, t: model(x, torch.full((n,), t, dtype=torch.long), lr, magnification_factor)


def sar_pred_fn(model, n, sar_img):
    return lambda x, t: model(x, torch.full((n,), t, dtype=torch.long), sar_img.unsqueeze(0))


def generation_pred_fn(model, n, target_class, cfg_scale):
    def fn(x, t):
        tt = torch.full((n,), t, dtype=torch.long)
        pred = model(x, tt, target_class)
        return O.lerp64(model(x, tt, None), pred, cfg_scale) if cfg_scale > 0 else pred
    return fn


def chain(kind, clip, pred_fn, shape, noise_steps, schedule, sampler, noise_source):
    """The float64 chain of `sampler` = ("ancestral",) | ("ddim", S, eta) | ("dpmpp_2m", S) with the model's output read as
    `kind`; `schedule` = (alpha, alpha_hat, beta) of oracle.diffusion_oracle.schedule."""
    alpha, alpha_hat, beta = schedule
    eps_fn = eps_fn_of(kind, clip, alpha_hat, pred_fn)
    if sampler[0] == "ddim":
        return O.chain(eps_fn, shape, noise_steps, alpha_hat, sampler[1], sampler[2], noise_source)
    if sampler[0] == "dpmpp_2m":
        return P.chain(eps_fn, shape, noise_steps, alpha_hat, sampler[1], noise_source)
    # the reference's ancestral loop (oracle.diffusion_oracle.sample) with a float64 state
    n = shape[0]
    x = noise_source(noise_steps, shape).double()
    a64, ah64, b64 = alpha.double(), alpha_hat.double(), beta.double()
    for i in reversed(range(1, noise_steps)):
        eps = eps_fn(x.float(), i)
        z = noise_source(i, shape).double() if i > 1 else torch.zeros_like(x)
        x = D.sampler_step(x, eps, z, torch.full((n,), i, dtype=torch.long), a64, ah64, b64)
    return x


# -- the Gaussian anchor in all three parameterisations (dpm_oracle: data N(0, VAR0) per pixel) -----------------------------------
def gauss_pred(kind, alpha_hat):
    """The optimal predictor of per-pixel N(0, VAR0) data, as eps, v or x0: pred(x, t) in float64, returned in x's dtype."""
    eps_of = P.gauss_eps(alpha_hat)

    def fn(x, t):
        return from_eps(kind, eps_of(x.double(), t), x, alpha_hat, t).to(x.dtype)
    return fn
