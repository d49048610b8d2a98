"""Float64 restatement of the training objective's contract (include/drs_hip.h: drs_diffusion_loss, drs_timestep_draw): the
difference d = pred - target is formed in fp32, as torch and the kernel form it; everything after that is float64.  Also the
bins (sums, counts, ring of the last `history` losses per bin) and the loss-aware draw."""
import math

import torch

KINDS = ("MSE", "MAE", "Huber")


def element_loss(d, kind, delta=1.0):
    """(l(d), l'(d)) of torch's mse_loss / l1_loss / huber_loss on a float64 tensor d."""
    if kind == "MSE":
        return d * d, 2.0 * d
    if kind == "MAE":
        return d.abs(), torch.sign(d)
    if kind == "Huber":
        inner = d.abs() < delta
        return (torch.where(inner, 0.5 * d * d, delta * (d.abs() - 0.5 * delta)),
                torch.where(d.abs() <= delta, d, delta * torch.sign(d)))
    raise ValueError(kind)


def image_weights(B, t=None, table=None, sample_w=None):
    """w_b = table[t_b] * sample_w[b] in float64; missing factors are 1."""
    w = torch.ones(B, dtype=torch.float64)
    if table is not None:
        w = w * table.double()[t]
    if sample_w is not None:
        w = w * sample_w.double()
    return w


def loss_and_grad(pred, target, kind, delta=1.0, w=None):
    """(per_image (B,), loss (), grad of pred's shape), all float64, for fp32 CPU tensors pred / target of shape (B, ...)."""
    assert pred.dtype == torch.float32 and target.dtype == torch.float32
    B = pred.shape[0]
    d = (pred - target).double().reshape(B, -1)  # the fp32 difference, widened
    n = d.shape[1]
    l, lp = element_loss(d, kind, delta)
    per_image = l.sum(dim=1) / n
    w = torch.ones(B, dtype=torch.float64) if w is None else w
    loss = (w * per_image).sum() / B
    grad = (w / (B * n))[:, None] * lp
    return per_image, loss, grad.reshape(pred.shape)


class BinsOracle:
    """bin(t) = t * nbins // T; per bin a sum and a count of the finite per-image losses, and the last `history` of them."""

    def __init__(self, T, nbins, history=10):
        self.T, self.nbins, self.history = T, nbins, history
        self.sum, self.count, self.nonfinite = [0.0] * nbins, [0] * nbins, 0
        self.ring = [[] for _ in range(nbins)]  # oldest first

    def update(self, per_image, t, ring=True):
        for v, tb in zip(per_image.tolist(), t.tolist()):
            if not math.isfinite(v):
                self.nonfinite += 1
                continue
            k = tb * self.nbins // self.T
            self.sum[k] += v
            self.count[k] += 1
            if ring:
                self.ring[k] = (self.ring[k] + [v])[-self.history:]

    def full(self):
        return all(len(r) == self.history for r in self.ring)


def bin_ranges(T, nbins):
    """Per bin (first valid timestep, number of timesteps 1 .. T - 1 in it)."""
    members = [[t for t in range(1, T) if t * nbins // T == k] for k in range(nbins)]
    return [(m[0], len(m)) for m in members]


def proposal(bins, eps=1e-3):
    """(p (nbins,), cumulative p) in float64, index order; None while a ring is not full."""
    if not bins.full():
        return None
    r = [math.sqrt(sum(v * v for v in ring) / len(ring)) for ring in bins.ring]
    total = 0.0
    for x in r:
        total += x
    p = [(1.0 - eps) * x / total + eps / bins.nbins if total > 0 else 1.0 / bins.nbins for x in r]
    cum, c = [], 0.0
    for x in p:
        c += x
        cum.append(c)
    return p, cum


def timestep_distribution(bins, eps=1e-3):
    """{t: (q(t), sample_w(t))} over t = 1 .. T - 1: the probability the draw gives t and the weight it hands out with it."""
    T, nbins = bins.T, bins.nbins
    prop = proposal(bins, eps)
    if prop is None:
        return {t: (1.0 / (T - 1), 1.0) for t in range(1, T)}
    p, _ = prop
    ranges = bin_ranges(T, nbins)
    return {t: (p[k] / ranges[k][1], ranges[k][1] / ((T - 1) * p[k]))
            for t in range(1, T) for k in [t * nbins // T]}


def draw(bins, u1, u2, eps=1e-3):
    """(t list, sample_w list) for fp32 uniforms u1, u2 (widened to float64 before any arithmetic)."""
    T, nbins = bins.T, bins.nbins
    prop = proposal(bins, eps)
    ts, ws = [], []
    ranges = bin_ranges(T, nbins)
    for a, b in zip(u1.double().tolist(), u2.double().tolist()):
        if prop is None:
            ts.append(1 + min(T - 2, math.floor(a * (T - 1))))
            ws.append(1.0)
            continue
        p, cum = prop
        k = next((j for j in range(nbins) if cum[j] > a), nbins - 1)
        first, cnt = ranges[k]
        ts.append(first + min(cnt - 1, math.floor(b * cnt)))
        ws.append(cnt / ((T - 1) * p[k]))
    return ts, ws


def draw_margins(bins, u1, u2, eps=1e-3):
    """Per sample (distance of u1 from the nearest CDF edge, distance of u2 * cnt_k from the nearest integer) for full rings:
    what a test uses to keep the pairs whose outcome does not hang on the last bits."""
    p, cum = proposal(bins, eps)
    ranges = bin_ranges(bins.T, bins.nbins)
    out = []
    for a, b in zip(u1.double().tolist(), u2.double().tolist()):
        k = next((j for j in range(bins.nbins) if cum[j] > a), bins.nbins - 1)
        x = b * ranges[k][1]
        out.append((min(abs(a - c) for c in cum), abs(x - round(x))))
    return out
