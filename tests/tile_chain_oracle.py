"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of the joint tile chain `split_aggregation_sampling.sample_scene` runs (aggregation="per_step"): one
state of scene size, cut into tiles at every reverse step, the tiles' noise predictions blended into one eps per scene
element by the Gaussian-weighted mean, then the ancestral step (`oracle.diffusion_oracle.sampler_step` on float64 tables)
or the DDIM step (`ddim_oracle.step`).  State, mean and update are float64; the model is called in fp32 per tile through
`eps_fn(x_tiles_fp32, t, (k0, k1))` -> (k1 - k0, C, S, S).  Tile coordinates and the weight plane are those of
`oracle.aggregation_oracle`.  Noise protocol of the product: x_T = noise_source(T, (1, C, Hs, Ws)), the noise of step i =
noise_source(i, (1, C, Hs, Ws)), none at the last ancestral step, and on a DDIM chain only when sigma > 0.
"""
import torch

import ddim_oracle as O
from oracle import diffusion_oracle as D


def gather(scene, infos):
    """(n, C, S, S): the windows (y0, y1, x0, x1) of a (C, Hs, Ws) scene."""
    return torch.stack([scene[:, y0:y1, x0:x1] for (y0, y1, x0, x1) in infos])


def blend(eps_tiles, infos, weight, height, width):
    """Float64 Gaussian-weighted mean of the tiles' eps per scene element: sum_k (w_k / sum_j w_j) * eps_k over the tiles
    that cover it.  Written with normalised weights so that an element one tile covers gets that tile's eps exactly."""
    C = eps_tiles.shape[1]
    w = weight.double()
    total = torch.zeros((height, width), dtype=torch.float64)
    for (y0, y1, x0, x1) in infos:
        total[y0:y1, x0:x1] += w
    assert torch.all(total != 0)
    out = torch.zeros((C, height, width), dtype=torch.float64)
    for k, (y0, y1, x0, x1) in enumerate(infos):
        out[:, y0:y1, x0:x1] += (w / total[y0:y1, x0:x1]) * eps_tiles[k].double()
    return out


def ancestral_step(x, eps, z, i, alpha, alpha_hat, beta):
    """`diffusion_oracle.sampler_step` with the fp32 tables widened to float64; z None = the zeros of the last step."""
    t = torch.full((x.shape[0],), i, dtype=torch.long)
    z = torch.zeros_like(x) if z is None else z.double()
    return D.sampler_step(x.double(), eps.double(), z, t, alpha.double(), alpha_hat.double(), beta.double())


def step(x, eps, z, i, i_prev, eta, alpha, alpha_hat, beta):
    """One move of a (1, C, H, W) float64 state given its eps: ancestral (i_prev None) or DDIM i -> i_prev."""
    if i_prev is None:
        return ancestral_step(x, eps, z, i, alpha, alpha_hat, beta)
    return O.step(x, eps, z, i, i_prev, eta, alpha_hat)


def moves(noise_steps, sampling_steps):
    """[(i, i_prev)] of a chain: i_prev None on the ancestral chain T - 1 .. 1."""
    if sampling_steps is None:
        return [(i, None) for i in range(noise_steps - 1, 0, -1)]
    taus = O.timesteps(noise_steps, sampling_steps)
    return list(zip(taus, taus[1:] + [0]))


def draws_noise(i, i_prev, eta):
    return i > 1 if i_prev is None else (eta > 0 and i_prev > 0)


def chain(eps_fn, channels, height, width, infos, weight, noise_steps, schedule, noise_source, sampling_steps=None,
          eta=0.0, keep=False):
    """The joint chain.  `schedule` = (alpha, alpha_hat, beta) fp32 tables; `infos` / `weight` from aggregation_oracle
    (super-resolved coordinates).  Returns the float64 (C, height, width) state after the last step (un-clamped), and with
    keep=True the list of states after every step."""
    alpha, alpha_hat, beta = schedule
    shape = (1, channels, height, width)
    x = noise_source(noise_steps, shape).double()
    states = []
    with torch.no_grad():
        for i, i_prev in moves(noise_steps, sampling_steps):
            tiles = gather(x[0].float(), infos)
            eps_tiles = eps_fn(tiles, i, (0, len(infos)))
            eps = blend(eps_tiles, infos, weight, height, width)[None]
            z = noise_source(i, shape) if draws_noise(i, i_prev, eta) else None
            x = step(x, eps, z, i, i_prev, eta, alpha, alpha_hat, beta)
            if keep:
                states.append(x[0].clone())
    return (x[0], states) if keep else x[0]


def tile_chain(eps_fn, k, channels, S, noise_steps, schedule, noise_source, sampling_steps=None, eta=0.0):
    """The independent chain of tile k alone (the final mode's protocol) in the same float64 arithmetic, with
    `noise_source(i, (1, C, S, S))`: what the joint chain must reduce to where tiles do not overlap."""
    alpha, alpha_hat, beta = schedule
    shape = (1, channels, S, S)
    x = noise_source(noise_steps, shape).double()
    with torch.no_grad():
        for i, i_prev in moves(noise_steps, sampling_steps):
            eps = eps_fn(x.float(), i, (k, k + 1))
            z = noise_source(i, shape) if draws_noise(i, i_prev, eta) else None
            x = step(x, eps, z, i, i_prev, eta, alpha, alpha_hat, beta)
    return x[0]


def unet_eps_fn(model, lr_tiles, magnification_factor):
    """eps_fn over `oracle.unet_oracle.OracleUNet` with one LR tile per SR tile: lr_tiles (n, C, ps, ps)."""
    def eps_fn(x_tiles, t, rng):
        k0, k1 = rng
        return model(x_tiles, torch.full((k1 - k0,), t, dtype=torch.long), lr_tiles[k0:k1], magnification_factor)
    return eps_fn
