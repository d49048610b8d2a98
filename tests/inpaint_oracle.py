"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of sampling with known pixels (RePaint, Lugmayr et al., CVPR 2022, Algorithm 1) as
`Diffusion.sample_known(..., known, known_mask, resample=, jump=)` runs it: the conditioned reverse move, the forward jump, the
move schedule and the chain for the three model calls, with the noise protocol of the product (x_T from `noise_source(T,
shape)`; a reverse move t -> t_prev draws `noise_source(t, shape)` iff t_prev > 0, whatever eta is; a forward jump to level t
draws `noise_source(t, shape)`).  The model calls run the CPU oracle UNets of `oracle.unet_oracle` in fp32; the chain state
and every update are float64.  Built on `ddim_oracle` (coefficients, step, lerp64) and on a float64 form of the ancestral
step of `oracle.diffusion_oracle.sampler_step`.
"""
import math

import torch

import ddim_oracle as O


def ancestral_coefficients(t, alpha, alpha_hat, beta):
    """(A, B, sigma) of x' = A x + B eps + sigma z for `oracle.diffusion_oracle.sampler_step`, in float64 from the fp32
    table entries: 1 / sqrt(a) * (x - (1 - a) / sqrt(1 - ah) * eps) + sqrt(b) * z."""
    a, ah, b = float(alpha[t]), float(alpha_hat[t]), float(beta[t])
    A = 1.0 / math.sqrt(a)
    return A, -A * (1.0 - a) / math.sqrt(1.0 - ah), math.sqrt(b)


def ancestral_step(x, eps, z, t, alpha, alpha_hat, beta):
    """One ancestral move t -> t - 1 in float64; z None adds nothing (the reference adds zeros at t = 1)."""
    A, B, sigma = ancestral_coefficients(t, alpha, alpha_hat, beta)
    out = A * x.double() + B * eps.double()
    return out if z is None else out + sigma * z.double()


def known_coefficients(t_prev, alpha_hat):
    """(a, b) of q(x_t_prev | known) = a known + b z."""
    ah = float(alpha_hat[t_prev])
    return math.sqrt(ah), math.sqrt(1.0 - ah)


def _mask(mask, like):
    m = mask != 0
    while m.dim() < like.dim():
        m = m.unsqueeze(0)
    return m.expand_as(like)


def move(x, eps, z, known, mask, t, t_prev, alpha_hat, eta=0.0, alpha=None, beta=None):
    """The conditioned reverse move t -> t_prev in float64: where mask == 0 the ancestral step (alpha and beta given; t_prev
    = t - 1) or the DDIM step; elsewhere `known` noised to level t_prev with the same z, or `known` itself at level 0."""
    if alpha is not None:
        assert t_prev == t - 1
        unknown = ancestral_step(x, eps, z, t, alpha, alpha_hat, beta)
    else:
        unknown = O.step(x, eps, z, t, t_prev, eta, alpha_hat)
    if t_prev == 0:
        kn = known.double().expand_as(unknown)
    else:
        a, b = known_coefficients(t_prev, alpha_hat)
        kn = a * known.double() + b * z.double()
    return torch.where(_mask(mask, unknown), kn, unknown)


def renoise_coefficients(s, t, alpha_hat):
    r = float(alpha_hat[t]) / float(alpha_hat[s])
    return math.sqrt(r), math.sqrt(1.0 - r)


def renoise(x, z, s, t, alpha_hat):
    """The forward jump from level s to level t > s in float64."""
    A, B = renoise_coefficients(s, t, alpha_hat)
    return A * x.double() + B * z.double()


def levels(noise_steps, sampling_steps):
    """The levels of the positions 0 .. S: T - 1 .. 1 (ancestral) or the DDIM timesteps, then 0."""
    taus = list(range(noise_steps - 1, 0, -1)) if sampling_steps is None else O.timesteps(noise_steps, sampling_steps)
    return taus + [0]


def schedule(S, resample, jump):
    """The walk over positions 0 .. S as [(p, q)]: position after position; a position p with 0 < p < S and p % jump == 0 is
    followed, `resample - 1` times, by the jump up to p - jump and the `jump` moves down to p again (those pass no other
    multiple of `jump`, so every such position is resampled on its first visit only)."""
    moves = []
    for p in range(1, S + 1):
        moves.append((p - 1, p))
        if p < S and p % jump == 0:
            block = [(p, p - jump)] + [(q, q + 1) for q in range(p - jump, p)]
            moves += block * (resample - 1)
    return moves


def chain(eps_fn, shape, noise_steps, alpha, alpha_hat, beta, sampling_steps, eta, noise_source, known, mask, resample=1,
          jump=1, model_dtype=torch.float32):
    """A chain with known pixels: eps_fn(x, t) -> predicted noise (fp32 or float64), x the state in `model_dtype` (the
    networks see fp32).  Returns the float64 result."""
    L = levels(noise_steps, sampling_steps)
    x = noise_source(noise_steps, shape).double()
    for p, q in schedule(len(L) - 1, resample, jump):
        t, t_to = L[p], L[q]
        if q < p:
            x = renoise(x, noise_source(t_to, shape), t, t_to, alpha_hat)
            continue
        eps = eps_fn(x.to(model_dtype), t)
        z = noise_source(t, shape) if t_to > 0 else None
        if sampling_steps is None:
            x = move(x, eps, z, known, mask, t, t_to, alpha_hat, alpha=alpha, beta=beta)
        else:
            x = move(x, eps, z, known, mask, t, t_to, alpha_hat, eta=eta)
    return x


def sample_superres(model, n, lr_img, noise_steps, sched, magnification_factor, image_size, sampling_steps, eta, noise_source,
                    known, mask, resample=1, jump=1, input_channels=3):
    """`Diffusion.sample_known` of train_diffusion_superres.py: `model` = oracle.unet_oracle.OracleUNet, `sched` =
    (alpha, alpha_hat, beta)."""
    lr = lr_img if lr_img.dim() == 4 else lr_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), lr, magnification_factor)
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, *sched, sampling_steps, eta, noise_source,
                 known, mask, resample, jump)


def sample_sar(model, n, sar_img, noise_steps, sched, image_size, sampling_steps, eta, noise_source, known, mask, resample=1,
               jump=1, ndvi_channels=1):
    """`Diffusion.sample_known` of train_diffusion_SAR_TO_NDVI.py: `model` = OracleUNetSAR."""
    sar = sar_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), sar)
    return chain(eps_fn, (n, ndvi_channels, image_size, image_size), noise_steps, *sched, sampling_steps, eta, noise_source,
                 known, mask, resample, jump)


def sample_generation(model, n, target_class, cfg_scale, noise_steps, sched, image_size, sampling_steps, eta, noise_source,
                      known, mask, resample=1, jump=1, input_channels=3):
    """`Diffusion.sample_known` of generate_new_imgs/train_diffusion_generation.py: `model` = OracleUNetGeneration; eps =
    lerp(uncond, cond, cfg_scale) for cfg_scale > 0."""
    def eps_fn(x, t):
        tt = torch.full((n,), t, dtype=torch.long)
        eps = model(x, tt, target_class)
        if cfg_scale > 0:
            eps = O.lerp64(model(x, tt, None), eps, cfg_scale)
        return eps
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, *sched, sampling_steps, eta, noise_source,
                 known, mask, resample, jump)
