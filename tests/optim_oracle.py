"""Float64 oracle of `optim.FusedAdamW` (csrc/optim.hip): torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW written out in
plain torch on float64 CPU tensors, plus the rule that a step whose global gradient norm is not finite is skipped - parameters
and moments untouched, the per-parameter step counts still advanced (what the device does, without asking the host)."""
import math

import torch


def global_norm(grads):
    """sqrt of the sum of squares over every gradient that is not None, in float64."""
    total = torch.zeros((), dtype=torch.float64)
    for g in grads:
        if g is not None:
            total = total + (g.double() ** 2).sum()
    return math.sqrt(total.item()) if total.item() >= 0 else float("nan")  # (a NaN total fails the comparison)


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s factor: min(1, max_norm / (norm + 1e-6)); 1 without clipping."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


class AdamWOracle:
    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, skip_nonfinite=True):
        self.p = [torch.as_tensor(p).detach().double().clone() for p in params]
        self.m = [None] * len(self.p)
        self.v = [None] * len(self.p)
        self.steps = [0] * len(self.p)
        self.betas, self.eps, self.weight_decay, self.max_norm = betas, eps, weight_decay, max_norm
        self.skip_nonfinite = skip_nonfinite
        self.skipped = 0
        self.last_norm = self.last_coef = None

    def step(self, grads, lr):
        """One step with `grads[i]` (None: that parameter is left alone, like torch) at learning rate `lr`."""
        b1, b2 = self.betas
        with_norm = self.max_norm is not None or self.skip_nonfinite
        norm = global_norm(grads) if with_norm else 0.0
        coef = clip_coef(norm, self.max_norm)
        self.last_norm, self.last_coef = norm, coef
        skip = self.skip_nonfinite and not math.isfinite(norm)
        self.skipped += int(skip)
        for i, g in enumerate(grads):
            if g is None:
                continue
            if self.m[i] is None:
                self.m[i], self.v[i] = torch.zeros_like(self.p[i]), torch.zeros_like(self.p[i])
            self.steps[i] += 1  # counted even when the step is skipped
            if skip:
                continue
            g = g.double() * coef
            self.p[i] = self.p[i] * (1.0 - lr * self.weight_decay)
            self.m[i] = self.m[i] + (1.0 - b1) * (g - self.m[i])
            self.v[i] = self.v[i] * b2 + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** self.steps[i], 1.0 - b2 ** self.steps[i]
            self.p[i] = self.p[i] - (lr / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + self.eps)
