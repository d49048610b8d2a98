"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of what `Diffusion(zero_terminal_snr=True)` and `guidance_rescale` add (Lin et al.,
"Common Diffusion Noise Schedules and Sample Steps Are Flawed", 2024): the rescaled schedule, the reverse move away from the
terminal level (alpha_hat == 0, where x_t is the noise and the network names x0 directly), the guidance rescale, and a chain that
takes the terminal move itself and hands every other move to the float64 moves of ddim_oracle, dpm_oracle, inpaint_oracle and
prediction_oracle / threshold_oracle.  Written from the definitions: q(x_s | x_t, x0) of the DDIM family at a_t = 0,
  x_s = a_s x0 + sqrt(1 - ah_s - sigma^2) x_t + sigma z,   sigma = eta sqrt(1 - ah_s)   (0 at s == 0)
whose eta = 1 member is the DDPM posterior at beta_t = 1 (mean a_s x0, variance 1 - ah_s).
"""
import math

import numpy as np
import torch

import ddim_oracle as O
import dpm_oracle as P
import inpaint_oracle as I
import prediction_oracle as PO
import threshold_oracle as TO


# -- the schedule ---------------------------------------------------------------------------------------------------------------
def rescale(alpha_hat):
    """ah' = ((s - s[T-1]) s[0] / (s[0] - s[T-1]))^2 with s = sqrt(ah), float64, nothing pinned."""
    s = torch.as_tensor(alpha_hat).double().sqrt()
    return ((s - s[-1]) * s[0] / (s[0] - s[-1])) ** 2


def schedule(kind, T):
    """(alpha, alpha_hat, beta) fp32 as `Diffusion(kind, ..., noise_steps=T, zero_terminal_snr=True)` holds them: the rescaled
    table of `oracle.diffusion_oracle.schedule`'s alpha_hat with both ends pinned, beta = 1 - ah_t / ah_{t-1} (beta_0 = 1 - ah_0)
    and alpha = 1 - beta in fp32."""
    from oracle import diffusion_oracle as D
    _, ah, _ = D.schedule(kind, T)
    out = rescale(ah).float()
    out[-1] = 0.0
    out[0] = ah[0]
    beta = torch.empty_like(out)
    beta[0] = 1 - out[0]
    beta[1:] = 1 - out[1:] / out[:-1]
    return 1.0 - beta, out, beta


def logsnr_levels(alpha_hat, S):
    """T - 1, then the S - 1 logSNR-spaced levels of the table without its terminal entry."""
    T = len(alpha_hat)
    return [T - 1] + (P.logsnr_levels(alpha_hat[:-1], S - 1) if S > 1 else [])


# -- the terminal move ----------------------------------------------------------------------------------------------------------
def lerp32(uncond, cond, w):
    """torch.lerp(uncond, cond, w) as the library's fp32 kernels form it for |w| >= 0.5: cond - fl(fl(cond - uncond) fl(1 - w)),
    every operation rounded to fp32."""
    assert abs(w) >= 0.5
    u, c = uncond.float().numpy(), cond.float().numpy()
    d = (c - u).astype(np.float32)
    return torch.from_numpy((c - (d * np.float32(np.float32(1.0) - np.float32(w))).astype(np.float32)).astype(np.float32))


def x0_of(kind, pred, clip=None, scale=None, pred_uncond=None, w=0.0):
    """The clean image the network names at the terminal level (float64): -v or the x0 prediction, guided (float64 lerp), then
    clamped to `clip`, or thresholded with the given per-image `scale` (n values; threshold_oracle's rule)."""
    assert kind in ("v", "x0")
    p = pred.double() if pred_uncond is None else O.lerp64(pred_uncond, pred, w)
    x0 = -p if kind == "v" else p
    if clip is None:
        return x0
    lo, hi = clip
    if scale is None:
        return torch.where(torch.isfinite(x0), x0.clamp(lo, hi), x0)
    c, r = TO.centre_and_half_range(clip)
    sv = torch.as_tensor(scale).double().view(-1, 1, 1, 1)
    dynamic = (sv > r) & torch.isfinite(sv)
    safe = torch.where(dynamic, sv, torch.ones_like(sv))
    d = x0 - c
    q_dyn = (c + (torch.minimum(torch.maximum(d, -safe), safe) / safe) * r).clamp(lo, hi)
    q = torch.where(dynamic, q_dyn, x0.clamp(lo, hi))
    return torch.where(torch.isfinite(x0), q, x0)


def terminal_coefficients(t_prev, eta, alpha_hat):
    """(c0, c1, sigma) in float64 from the fp32 table entry of t_prev (eta as the fp32 value the library is handed)."""
    ap, eta = float(alpha_hat[t_prev]), float(np.float32(eta))
    sigma = 0.0 if t_prev == 0 else eta * math.sqrt(max(1.0 - ap, 0.0))
    return math.sqrt(ap), math.sqrt(max((1.0 - ap) * (1.0 - eta * eta), 0.0)), sigma


def terminal_step(x, pred, z, t_prev, alpha_hat, kind, eta=0.0, clip=None, scale=None, pred_uncond=None, w=0.0, known=None,
                  mask=None):
    """(x', x0, terms): the move from the terminal level to t_prev of the float64 state x, the x0 it used, and the sum of the
    absolute terms of the update per element (the scale an fp32 evaluation's rounding is measured against).  Where `mask` is
    nonzero the element is `known` forward-noised to t_prev with the same z (`known` itself at level 0)."""
    c0, c1, sigma = terminal_coefficients(t_prev, eta, alpha_hat)
    x0 = x0_of(kind, pred, clip, scale, pred_uncond, w)
    x = x.double()
    out, terms = c0 * x0 + c1 * x, (c0 * x0).abs() + (c1 * x).abs()
    if sigma != 0.0:
        out, terms = out + sigma * z.double(), terms + (sigma * z.double()).abs()
    if known is not None:
        if t_prev == 0:
            kn = known.double().expand_as(out)
        else:
            a, b = I.known_coefficients(t_prev, alpha_hat)
            kn = a * known.double() + b * z.double()
        out = torch.where(I._mask(mask, out), kn, out)
    return out, x0, terms


# -- guidance rescale -----------------------------------------------------------------------------------------------------------
def cfg_rescale(cond, uncond, w, phi):
    """(out, f): g f per image with g = the fp32 lerp the library forms (`lerp32`) and f = 1 + phi (std(cond) / std(g) - 1) in
    float64, both standard deviations over the image's elements; std(g) == 0 or a ratio that is not finite: f = 1."""
    g = lerp32(uncond, cond, w).double()
    sc, sg = cond.double().flatten(1).std(dim=1, unbiased=False), g.flatten(1).std(dim=1, unbiased=False)
    ratio = sc / torch.where(sg == 0, torch.ones_like(sg), sg)
    f = torch.where((sg == 0) | ~torch.isfinite(ratio), torch.ones_like(sg), 1.0 + float(np.float32(phi)) * (ratio - 1.0))
    return g * f.view(-1, *([1] * (g.dim() - 1))), f


def guided_pred_fn(cond_fn, uncond_fn, w, phi):
    """pred_fn(x, t) of a guided sampler: the float64 lerp for phi == 0, `cfg_rescale` of the two fp32 outputs otherwise."""
    def fn(x, t):
        c, u = cond_fn(x, t), uncond_fn(x, t)
        return O.lerp64(u, c, w) if phi == 0 else cfg_rescale(c, u, w, phi)[0]
    return fn


# -- the chain ------------------------------------------------------------------------------------------------------------------
def chain(kind, clip, pred_fn, shape, noise_steps, sched, sampler, noise_source, threshold=None, known=None, mask=None,
          resample=1, jump=1, model_dtype=torch.float32):
    """The float64 chain of `sampler` = ("ancestral",) | ("ddim", S, eta) | ("dpmpp_2m", S) on a zero-terminal-SNR `sched` =
    (alpha, alpha_hat, beta), the model's output pred_fn(x, t) read as `kind` ("v" | "x0"), with the product's noise protocol
    (x_T from noise_source(T, shape); a reverse move t -> t_to draws noise_source(t, shape) iff it ends above level 0 and is
    ancestral, has known pixels or eta > 0; a forward jump to t_to draws noise_source(t_to, shape)).  A move away from level
    T - 1 is `terminal_step` (the ancestral chain's with eta = 1; under dpmpp_2m the next move is first order); every other move
    is the float64 move of the oracle that owns it, on the eps `prediction_oracle.to_eps` / `threshold_oracle.to_eps` make of
    the prediction."""
    alpha, alpha_hat, beta = sched
    T = noise_steps
    assert float(alpha_hat[T - 1]) == 0.0 and kind in ("v", "x0")
    ancestral, dpm = sampler[0] == "ancestral", sampler[0] == "dpmpp_2m"
    eta = sampler[2] if sampler[0] == "ddim" else 0.0
    if ancestral:
        lv = list(range(T - 1, 0, -1))
    else:
        lv = logsnr_levels(alpha_hat, sampler[1]) if dpm else O.timesteps(T, sampler[1])
    L = lv + [0]
    x = noise_source(T, shape).double()
    x0_prev, hist_level = None, None
    for p, q in I.schedule(len(L) - 1, resample, jump):
        t, t_to = L[p], L[q]
        if q < p:
            x = I.renoise(x, noise_source(t_to, shape), t, t_to, alpha_hat)
            continue
        xs = x.to(model_dtype)
        pred = pred_fn(xs, t)
        z = noise_source(t, shape) if t_to > 0 and (known is not None or ancestral or eta > 0) else None
        if t == T - 1:
            scale = None
            if threshold is not None:
                scale = TO.scales_of(x0_of(kind, pred), clip, threshold)
            x, x0_prev, _ = terminal_step(x, pred, z, t_to, alpha_hat, kind, 1.0 if ancestral else eta, clip, scale, known=known,
                                          mask=mask)
            hist_level = None
            continue
        if threshold is not None:
            eps = TO.to_eps(kind, pred, xs, alpha_hat, t, clip, threshold)[0]
        else:
            eps = PO.to_eps(kind, pred, xs, alpha_hat, t, clip)[0]
        if dpm:
            second = t_to > 0 and hist_level is not None and hist_level == L[p - 1]
            x, x0_prev = P.step(x, eps, x0_prev, hist_level if second else None, t, t_to, alpha_hat)
            hist_level = t
        elif known is not None:
            if ancestral:
                x = I.move(x, eps, z, known, mask, t, t_to, alpha_hat, alpha=alpha, beta=beta)
            else:
                x = I.move(x, eps, z, known, mask, t, t_to, alpha_hat, eta=eta)
        elif ancestral:
            x = I.ancestral_step(x, eps, z, t, alpha, alpha_hat, beta)
        else:
            x = O.step(x, eps, z, t, t_to, eta, alpha_hat)
    return x


# -- the Gaussian anchor with a mean: data N(MU, VAR0) per pixel ----------------------------------------------------------------
MU, VAR0 = 0.4, P.VAR0


def gauss_pred(kind, alpha_hat):
    """The optimal predictor of per-pixel N(MU, VAR0) data as v or x0, float64, returned in x's dtype: x_t is N(a MU, ah VAR0 +
    1 - ah), E[x0 | x_t] = MU + a VAR0 (x_t - a MU) / var_t, eps = (x_t - a x0) / s, v = a eps - s x0 (at a == 0: x0 = MU,
    v = -MU)."""
    def fn(x, t):
        ah = float(alpha_hat[t])
        a, s = math.sqrt(ah), math.sqrt(1.0 - ah)
        xd = x.double()
        x0 = MU + a * VAR0 * (xd - a * MU) / (ah * VAR0 + 1.0 - ah)
        out = x0 if kind == "x0" else a * (xd - a * x0) / s - s * x0
        return out.to(x.dtype)
    return fn


def gauss_exact(x_T, alpha_hat):
    """Where the probability-flow ODE takes x_T (level T - 1, N(0, 1)) to level 0: a_0 MU + sqrt(var_0) x_T."""
    ah0 = float(alpha_hat[0])
    return math.sqrt(ah0) * MU + math.sqrt(ah0 * VAR0 + 1.0 - ah0) * x_T.double()


def gauss_chain_error(alpha_hat, S, kind="v", shape=(1, 1, 4, 4), seed=0):
    """rel-L2 of the float64 DDIM eta = 0 chain of S levels on the Gaussian problem against `gauss_exact` (predictor in float64)."""
    T = len(alpha_hat)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    got = chain(kind, None, gauss_pred(kind, alpha_hat), shape, T, (None, alpha_hat, None), ("ddim", S, 0.0),
                lambda i, s: x_T, model_dtype=torch.float64)
    want = gauss_exact(x_T, alpha_hat)
    return ((got - want).norm() / want.norm()).item()
