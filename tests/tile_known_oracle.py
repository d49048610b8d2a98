"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of the joint tile chain with known pixels, as `split_aggregation_sampling.sample_scene(..., known=,
known_mask=, resample=, jump=)` runs it, composed from the oracles of its parts: the scene is cut into tiles and the tiles'
noise predictions blended as in `tile_chain_oracle` (gather, blend), the levels and the walk over them are those of
`inpaint_oracle` (levels, schedule), a reverse move is its conditioned `move` on the scene state - the ancestral or DDIM step
where the mask is zero, `known` noised to the level reached elsewhere - and a forward jump its `renoise`.  Noise protocol of
the product: x_T = noise_source(T, (1, C, Hs, Ws)); a reverse move t -> t_prev draws noise_source(t, scene shape) iff t_prev >
0, whatever eta is; a jump to level t draws noise_source(t, scene shape).  The model is called in fp32 per tile through
`eps_fn(x_tiles_fp32, t, (k0, k1))`, as in `tile_chain_oracle.chain`.
"""
import torch

import inpaint_oracle as I
import tile_chain_oracle as TC


def chain(eps_fn, channels, height, width, infos, weight, noise_steps, schedule, noise_source, known, mask,
          sampling_steps=None, eta=0.0, resample=1, jump=1, record=None):
    """The joint chain with known pixels: the float64 (C, height, width) state after the last move (un-clamped).  `schedule` =
    (alpha, alpha_hat, beta) fp32 tables; `known` (C, height, width); `mask` (height, width) or (1 | C, height, width),
    nonzero = known.  `record`, a list, receives one ("move" | "jump", t, t_to, drew) per move."""
    alpha, alpha_hat, beta = schedule
    shape = (1, channels, height, width)
    L = I.levels(noise_steps, sampling_steps)
    x = noise_source(noise_steps, shape).double()
    with torch.no_grad():
        for p, q in I.schedule(len(L) - 1, resample, jump):
            t, t_to = L[p], L[q]
            if q < p:
                x = I.renoise(x, noise_source(t_to, shape), t, t_to, alpha_hat)
                if record is not None:
                    record.append(("jump", t, t_to, t_to))
                continue
            tiles = TC.gather(x[0].float(), infos)
            eps = TC.blend(eps_fn(tiles, t, (0, len(infos))), infos, weight, height, width)[None]
            z = noise_source(t, shape) if t_to > 0 else None
            if sampling_steps is None:
                x = I.move(x, eps, z, known, mask, t, t_to, alpha_hat, alpha=alpha, beta=beta)
            else:
                x = I.move(x, eps, z, known, mask, t, t_to, alpha_hat, eta=eta)
            if record is not None:
                record.append(("move", t, t_to, t if z is not None else None))
    return x[0]


def block_mask(seed, height, width, block=8, p=0.5):
    """A seeded (height, width) bool mask of `block` x `block` squares, each known with probability p."""
    gen = torch.Generator().manual_seed(seed)
    gh, gw = -(-height // block), -(-width // block)
    coarse = torch.rand((gh, gw), generator=gen) < p
    return coarse.repeat_interleave(block, 0).repeat_interleave(block, 1)[:height, :width].contiguous()


def check_mask(mask, infos, lo=0.3, hi=0.7):
    """The known fraction of a (H, W) mask is in [lo, hi] and every tile window holds known and unknown pixels."""
    frac = mask.double().mean().item()
    assert lo <= frac <= hi, frac
    for (y0, y1, x0, x1) in infos:
        win = mask[y0:y1, x0:x1]
        assert win.any() and not win.all(), (y0, x0)
    return frac
