"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of the DDIM sampler (Song et al., "Denoising Diffusion Implicit Models", eq. 12) that
`Diffusion.sample(..., sampling_steps=S, eta=eta)` runs: the step, the timestep list and the chain, with the noise protocol
of the product (x_T from `noise_source(T, shape)`, the noise of the move tau_k -> tau_{k-1} from `noise_source(tau_k,
shape)`, drawn only when sigma > 0).  The model calls run the CPU oracle UNets of `oracle.unet_oracle` in fp32; the chain
state and the update are float64.
"""
import math

import torch


def timesteps(noise_steps, sampling_steps):
    """Descending: T - 1 .. 1 on an integer stride; [T - 1] for one step."""
    T, S = noise_steps, sampling_steps
    assert 1 <= S <= T - 1
    if S == 1:
        return [T - 1]
    return sorted({1 + (k * (T - 2)) // (S - 1) for k in range(S)}, reverse=True)


def coefficients(t, t_prev, eta, alpha_hat):
    """(A, B, sigma) of x' = A x + B eps + sigma z, in float64 from the fp32 table entries."""
    at, ap = float(alpha_hat[t]), float(alpha_hat[t_prev])
    sigma = 0.0 if t_prev == 0 else eta * math.sqrt((1 - ap) / (1 - at)) * math.sqrt(1 - at / ap)
    A = math.sqrt(ap / at)
    B = math.sqrt(max(1 - ap - sigma * sigma, 0.0)) - math.sqrt(ap) * math.sqrt(1 - at) / math.sqrt(at)
    return A, B, sigma


def step(x, eps, z, t, t_prev, eta, alpha_hat):
    """One DDIM move t -> t_prev in float64; z may be None when sigma == 0."""
    A, B, sigma = coefficients(t, t_prev, eta, alpha_hat)
    out = A * x.double() + B * eps.double()
    if sigma > 0:
        out = out + sigma * z.double()
    return out


def lerp64(uncond, cond, w):
    """torch.lerp(uncond, cond, w) in float64."""
    return uncond.double() + w * (cond.double() - uncond.double())


def chain(eps_fn, shape, noise_steps, alpha_hat, sampling_steps, eta, noise_source, keep=False):
    """A DDIM chain: eps_fn(x_fp32, t) -> predicted noise.  Returns the float64 result (and the list of states after every
    step with keep=True)."""
    taus = timesteps(noise_steps, sampling_steps)
    x = noise_source(noise_steps, shape).double()
    states = []
    for k, t in enumerate(taus):
        tp = taus[k + 1] if k + 1 < len(taus) else 0
        eps = eps_fn(x.float(), t)
        z = noise_source(t, shape) if (eta > 0 and tp > 0) else None
        x = step(x, eps, z, t, tp, eta, alpha_hat)
        if keep:
            states.append(x.clone())
    return (x, states) if keep else x


def sample_superres(model, n, lr_img, noise_steps, alpha_hat, magnification_factor, image_size, sampling_steps, eta,
                    noise_source, input_channels=3):
    """`Diffusion.sample` of train_diffusion_superres.py with sampling_steps: `model` = oracle.unet_oracle.OracleUNet;
    lr_img (C, h, w) broadcast over the n chains, or (n, C, h, w) one per chain."""
    lr = lr_img if lr_img.dim() == 4 else lr_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), lr, magnification_factor)
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, eta,
                 noise_source)


def sample_sar(model, n, sar_img, noise_steps, alpha_hat, image_size, sampling_steps, eta, noise_source, ndvi_channels=1):
    """`Diffusion.sample` of train_diffusion_SAR_TO_NDVI.py with sampling_steps: `model` = OracleUNetSAR."""
    sar = sar_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), sar)
    return chain(eps_fn, (n, ndvi_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, eta,
                 noise_source)


def sample_generation(model, n, target_class, cfg_scale, noise_steps, alpha_hat, image_size, sampling_steps, eta,
                      noise_source, input_channels=3):
    """`Diffusion.sample` of generate_new_imgs/train_diffusion_generation.py with sampling_steps: `model` =
    OracleUNetGeneration; eps = lerp(uncond, cond, cfg_scale) for cfg_scale > 0."""
    def eps_fn(x, t):
        tt = torch.full((n,), t, dtype=torch.long)
        eps = model(x, tt, target_class)
        if cfg_scale > 0:
            eps = lerp64(model(x, tt, None), eps, cfg_scale)
        return eps
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, eta,
                 noise_source)
