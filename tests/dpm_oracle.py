"""TEST INFRASTRUCTURE — NOT PART OF THE PRODUCT PATH.

Float64 restatement of DPM-Solver++(2M) (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic
Models", 2022, Algorithm 2, data prediction) on logSNR-spaced levels, as `Diffusion.sample(..., sampling_steps=S,
solver="dpmpp_2m")` runs it: the level list, the move, the chain (x_T from `noise_source(T, shape)`, nothing else drawn) and
the analytic Gaussian problem the anchor tests use.  The model calls run the CPU oracle UNets of `oracle.unet_oracle` in fp32;
the chain state, the history and the update are float64.  The move is written from the paper's exponential-integrator form
with logarithms for h, not from the product's E = (s_p / a_p)(a_t / s_t).
"""
import math

import torch

import ddim_oracle as O


def lam(alpha_hat, t):
    ah = float(alpha_hat[t])
    return 0.5 * math.log(ah / (1.0 - ah))


def logsnr_levels(alpha_hat, S):
    """S distinct descending levels in [1, T - 1]: nearest level to each of S uniform logSNR targets (ties: the larger t),
    pushed apart going down, then lifted to at least S - k going back up."""
    T = len(alpha_hat)
    assert 1 <= S <= T - 1
    lams = [lam(alpha_hat, t) for t in range(1, T)]
    lo, hi = lams[-1], lams[0]
    ts = []
    for k in range(S):
        # S uniform targets from lo to hi, both ends exact
        target = hi if (k == S - 1 and S > 1) else (lo if k == 0 else lo + k * ((hi - lo) / (S - 1)))
        best, best_d = None, None
        for t in range(T - 1, 0, -1):  # from the larger t: a later equal distance does not replace it
            d = abs(lams[t - 1] - target)
            if best_d is None or d < best_d:
                best, best_d = t, d
        ts.append(best)
    for k in range(1, S):
        ts[k] = min(ts[k], ts[k - 1] - 1)
    for k in range(S - 1, -1, -1):
        ts[k] = max(ts[k], S - k)
    return ts


def levels(alpha_hat, S, spacing):
    return logsnr_levels(alpha_hat, S) if spacing == "logsnr" else O.timesteps(len(alpha_hat), S)


def coefficients(t_q, t, t_p, alpha_hat):
    """(cx, ce, A, B, C) of x0 = cx x + ce eps, x' = A x + B eps + C x0_prev in float64 from the fp32 table entries; t_q None
    or -1: a first-order move.  The move to level 0 is first order and takes no logarithm (alpha_hat[0] may be 1)."""
    aht, ahp = float(alpha_hat[t]), float(alpha_hat[t_p])
    a_t, s_t, a_p, s_p = math.sqrt(aht), math.sqrt(1 - aht), math.sqrt(ahp), math.sqrt(max(1 - ahp, 0.0))
    second = t_q is not None and t_q >= 0
    if t_p == 0:
        assert not second
        e_mh = (s_p / a_p) * (a_t / s_t)  # exp(-h) with h = lam_0 - lam_t, which may be infinite
    else:
        e_mh = math.exp(-(lam(alpha_hat, t_p) - lam(alpha_hat, t)))
    phi = a_p * (1.0 - e_mh)
    k0, C = phi, 0.0
    if second:
        r = (lam(alpha_hat, t) - lam(alpha_hat, t_q)) / (lam(alpha_hat, t_p) - lam(alpha_hat, t))
        k0, C = phi * (1 + 1 / (2 * r)), -phi / (2 * r)
    return 1 / a_t, -s_t / a_t, s_p / s_t + k0 / a_t, -k0 * s_t / a_t, C


def gain(t_q, t, t_p, alpha_hat):
    """1 + 1 / r of a second-order move: the factor by which it amplifies an error of eps more than the first-order (DDIM)
    move does, through k0 = phi (1 + 1 / (2 r)) on the new and C = -phi / (2 r) on the previous prediction."""
    r = (lam(alpha_hat, t) - lam(alpha_hat, t_q)) / (lam(alpha_hat, t_p) - lam(alpha_hat, t))
    return 1 + 1 / r


def step(x, eps, x0_prev, t_q, t, t_p, alpha_hat):
    """One move t -> t_p in float64: (x', x0)."""
    cx, ce, A, B, C = coefficients(t_q, t, t_p, alpha_hat)
    x, eps = x.double(), eps.double()
    x0 = cx * x + ce * eps
    out = A * x + B * eps
    if C != 0.0:
        out = out + C * x0_prev.double()
    return out, x0


def chain_on(eps_fn, x, lv, alpha_hat, solver="dpmpp_2m", keep=False, model_dtype=torch.float32):
    """The chain from the float64 state x over the levels `lv` (then 0): eps_fn(x as `model_dtype`, t) -> predicted noise;
    `solver` "ddim" takes the same levels with the float64 DDIM eta = 0 move."""
    x0_prev, states = None, []
    for k, t in enumerate(lv):
        tp = lv[k + 1] if k + 1 < len(lv) else 0
        eps = eps_fn(x.to(model_dtype), t)
        if solver == "dpmpp_2m":
            t_q = lv[k - 1] if k > 0 and tp > 0 else None
            x, x0_prev = step(x, eps, x0_prev, t_q, t, tp, alpha_hat)
        else:
            x = O.step(x, eps, None, t, tp, 0.0, alpha_hat)
        if keep:
            states.append(x.clone())
    return (x, states) if keep else x


def chain(eps_fn, shape, noise_steps, alpha_hat, sampling_steps, noise_source, solver="dpmpp_2m", spacing="logsnr", keep=False):
    return chain_on(eps_fn, noise_source(noise_steps, shape).double(), levels(alpha_hat, sampling_steps, spacing), alpha_hat,
                    solver, keep)


def max_gain(alpha_hat, lv):
    """max_k (1 + 1 / r_k) over the second-order moves of the chain on the levels `lv`."""
    return max([gain(lv[k - 1], lv[k], lv[k + 1], alpha_hat) for k in range(1, len(lv) - 1)], default=1.0)


# -- the Gaussian anchor: data N(0, VAR0), so x_t is N(0, ah_t VAR0 + 1 - ah_t) and eps(x, t) is linear in x ------------------
VAR0 = 0.25


def gauss_var(alpha_hat, t):
    ah = float(alpha_hat[t])
    return ah * VAR0 + 1 - ah


def gauss_eps(alpha_hat):
    """eps(x, t) = x s_t / (ah_t VAR0 + 1 - ah_t), evaluated in float64 and returned in x's dtype."""
    def fn(x, t):
        return (x.double() * math.sqrt(1 - float(alpha_hat[t])) / gauss_var(alpha_hat, t)).to(x.dtype)
    return fn


def gauss_exact(x_start, alpha_hat, t_start):
    """Where the probability-flow ODE takes x_start from level t_start to level 0: x sqrt(var_0 / var_start)."""
    return x_start.double() * math.sqrt(gauss_var(alpha_hat, 0) / gauss_var(alpha_hat, t_start))


def gauss_chain_error(alpha_hat, S, solver, spacing="logsnr"):
    """Relative error of the float64 chain's end point on the Gaussian problem (scalar state, eps in float64 too)."""
    lv = levels(alpha_hat, S, spacing)
    x = torch.ones((), dtype=torch.float64)
    got = chain_on(gauss_eps(alpha_hat), x, lv, alpha_hat, solver, model_dtype=torch.float64)
    want = gauss_exact(x, alpha_hat, lv[0])
    return abs((got - want) / want).item()


# -- the three samplers --------------------------------------------------------------------------------------------------------
def sample_superres(model, n, lr_img, noise_steps, alpha_hat, magnification_factor, image_size, sampling_steps, noise_source,
                    input_channels=3):
    lr = lr_img if lr_img.dim() == 4 else lr_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), lr, magnification_factor)
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, noise_source)


def sample_sar(model, n, sar_img, noise_steps, alpha_hat, image_size, sampling_steps, noise_source, ndvi_channels=1):
    sar = sar_img.unsqueeze(0)

    def eps_fn(x, t):
        return model(x, torch.full((n,), t, dtype=torch.long), sar)
    return chain(eps_fn, (n, ndvi_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, noise_source)


def sample_generation(model, n, target_class, cfg_scale, noise_steps, alpha_hat, image_size, sampling_steps, noise_source,
                      input_channels=3):
    def eps_fn(x, t):
        tt = torch.full((n,), t, dtype=torch.long)
        eps = model(x, tt, target_class)
        if cfg_scale > 0:
            eps = O.lerp64(model(x, tt, None), eps, cfg_scale)
        return eps
    return chain(eps_fn, (n, input_channels, image_size, image_size), noise_steps, alpha_hat, sampling_steps, noise_source)
