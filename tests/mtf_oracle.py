"""TEST INFRASTRUCTURE - float64 numpy restatement of the sensor-MTF degradation, independent of
diffusionremotesensing_amd/mtf.py: the taps of a Nyquist gain, the dense one-axis matrix, the FIR form with clamped indices, the
noise / clamp epilogue and, per band, the projection of tests/consistency_oracle.py (imported, not restated).

The FIR bound.  An output is two nested chains of n_x and n_y fused multiply-adds on fp32 taps (which the oracle uses as they
are: no tap-rounding term): `fir_abs` runs them on absolute values, M bounds every partial sum, and an fp32 evaluation differs
from the exact one by at most M (n_y + n_x + 4) 2^-24 to first order; FIR_GAMMA doubles that as margin."""
import math

import numpy as np

import consistency_oracle as CO


def fir_gamma(n_y, n_x):
    return (n_y + n_x + 4) * 2.0 ** -24 * 2


def sigma_of(g, m):
    """The Gaussian whose transfer function exp(-2 pi^2 sigma^2 f^2) is g at f = 1 / (2 m)."""
    return m * math.sqrt(-2.0 * math.log(g)) / math.pi


def taps(g, m):
    """(k, L): n = 2 L + m weights exp(-(u - L - (m - 1) / 2)^2 / (2 sigma^2)), normalised in float64, rounded to fp32."""
    s = sigma_of(g, m)
    L = int(math.ceil(3.0 * s))
    d = np.arange(2 * L + m) - L - (m - 1) / 2.0
    k = np.exp(-d * d / (2.0 * s * s))
    return (k / k.sum()).astype(np.float32).astype(np.float64), L


def band_taps(gains, m):
    """(rows (n_ops, n), L, band_op): one row per distinct gain in order of first appearance, centred in the widest window."""
    distinct = []
    for g in gains:
        if g not in distinct:
            distinct.append(g)
    per = [taps(g, m) for g in distinct]
    L = max(l for _, l in per)
    rows = np.zeros((len(per), 2 * L + m))
    for r, (k, l) in enumerate(per):
        rows[r, L - l:L - l + k.shape[0]] = k
    return rows, L, [distinct.index(g) for g in gains]


def dtft_gain(k, m):
    """|sum_u k[u] exp(-2 pi i u / (2 m))|: the taps' gain at the LR Nyquist frequency."""
    return abs(np.sum(k * np.exp(-1j * np.pi * np.arange(k.shape[0]) / m)))


def dense(n_in, n_out, k, L, m):
    A = np.zeros((n_out, n_in))
    for i in range(n_out):
        for u in range(k.shape[0]):
            A[i, min(max(i * m + u - L, 0), n_in - 1)] += k[u]
    return A


def fir(x, k_y, k_x, L_y, L_x, m, h=None, w=None):
    """out[.., i, j] = sum_u k_y[u] sum_v k_x[v] x[.., clip(i m + u - L_y), clip(j m + v - L_x)] over the trailing two axes."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    h, w = H // m if h is None else h, W // m if w is None else w
    iy = np.clip(np.arange(h)[:, None] * m + np.arange(k_y.shape[0])[None] - L_y, 0, H - 1)  # (h, n_y)
    ix = np.clip(np.arange(w)[:, None] * m + np.arange(k_x.shape[0])[None] - L_x, 0, W - 1)  # (w, n_x)
    t = (x[..., :, ix] * k_x).sum(axis=-1)           # (.., H, w)
    return (np.moveaxis(t[..., iy, :], -2, -1) * k_y).sum(axis=-1)  # (.., h, w)


def fir_abs(x, k_y, k_x, L_y, L_x, m, h=None, w=None):
    return fir(np.abs(x), np.abs(k_y), np.abs(k_x), L_y, L_x, m, h, w)


def fir_bands(x, rows_y, rows_x, band_op, L_y, L_x, m):
    """(out, bound) for x (B, C, H, W): band c through rows[band_op[c]]."""
    out = np.stack([fir(x[:, c], rows_y[o], rows_x[o], L_y, L_x, m) for c, o in enumerate(band_op)], axis=1)
    mag = np.stack([fir_abs(x[:, c], rows_y[o], rows_x[o], L_y, L_x, m) for c, o in enumerate(band_op)], axis=1)
    return out, fir_gamma(rows_y.shape[1], rows_x.shape[1]) * mag


def epilogue(v, bound, z=None, sigma=None, clamp=False):
    """(v + sigma_c z, clamped into [0, 1] last; its bound: the FIR's plus 2^-24 |sigma z| for the one rounding of the fma)."""
    if z is not None:
        add = np.asarray(sigma, np.float64)[None, :, None, None] * np.asarray(z, np.float64)
        v, bound = v + add, bound + 2.0 ** -24 * np.abs(add)
    return (np.clip(v, 0.0, 1.0) if clamp else v), bound


class BandProjection:
    """tests/consistency_oracle.py's `Projection`, one per band: the per-band loop of every method the GPU tests compare with."""

    def __init__(self, H, W, m, gains, damping, lr_hw=None):
        h, w = (H // m, W // m) if lr_hw is None else lr_hw
        made = {}
        for g in gains:
            if g not in made:
                k, L = taps(g, m)
                made[g] = CO.Projection(dense(H, h, k, L, m), dense(W, w, k, L, m), damping)
        self.per_band = [made[g] for g in gains]

    def _each(self, f, *arrays):
        outs = [f(p, *(a[:, c] for a in arrays)) for c, p in enumerate(self.per_band)]
        if isinstance(outs[0], tuple):
            return tuple(np.stack([o[i] for o in outs], axis=1) for i in range(len(outs[0])))
        return np.stack(outs, axis=1)

    def degrade(self, x):
        """(A_c x_c, the section-28 bound of the dense evaluation)."""
        return self._each(lambda p, xc: (p.degrade(xc), p.gamma * p.degrade_abs(xc)), x)

    def project(self, x, y, strength=1.0):
        return self._each(lambda p, xc, yc: p.project(xc, yc, strength), x, y)

    def project_eps(self, eps, x, ah, y, strength=1.0):
        def one(p, ec, xc, yc):
            out, bound = p.project_eps(ec[:, None], xc[:, None], ah, yc[:, None], strength)
            return out[:, 0], bound[:, 0]
        return self._each(one, eps, x, y)
