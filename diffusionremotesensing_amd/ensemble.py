"""Statistics and scores of an ensemble: N samples of one conditional distribution, drawn by `Diffusion.sample_ensemble`
(or stacked by hand, e.g. from N tiler runs over one scene).

`members` is (N, B, C, H, W) fp32 on a ROCm device, member axis first, 2 <= N <= 32, and `truth` (B, C, H, W); (N, C, H, W)
members with a (C, H, W) truth are taken as B = 1.  `clamp=(lo, hi)` clamps members and truth first (torch.clamp: a NaN
stays a NaN).  Everything per element is one HIP launch that reads the members once and sorts the N values of an element in
registers (csrc/ensemble.hip through `hip_ops.ensemble_stats` / `hip_ops.ensemble_scores`; there is no CPU path).  With the
sorted members s_0 <= ... <= s_{N-1} of an element and its truth y:

    mean      sum(s) / N: the MMSE estimate
    std       sqrt(sum (s_i - mean)^2 / (N - 1))
    quantile  torch's interpolation='linear': pos = q (N - 1), k = floor(pos), s_k + (pos - k) (s_{min(k+1,N-1)} - s_k)
    CRPS      1/N sum |s_i - y| - 1/N^2 sum_i (2 i - N + 1) s_i   (= 1/N sum |x_i - y| - 1/(2 N^2) sum_ij |x_i - x_j|)
    rank      #{i : x_i < y}, 0 .. N

Sums, interpolation and CRPS are formed in float64 over the sorted order and rounded to fp32 once, in the maps; the
per-image scores come from the float64 values.  An element with a NaN member (or truth) is NaN in its maps, is left out of the
rank histogram and makes its image's scores NaN.
"""
import math

import torch

from . import hip_ops


def _batched(members, truth=None):
    """((N, B, C, H, W) members, (B, C, H, W) truth or None, whether a batch axis was added)."""
    if isinstance(members, torch.Tensor) and members.dim() == 4 and (truth is None or truth.dim() == 3):
        return members.unsqueeze(1), (truth.unsqueeze(0) if truth is not None else None), True
    return members, truth, False


def ensemble_statistics(members, quantiles=(0.05, 0.5, 0.95), clamp=None):
    """{"mean", "std", "quantiles"}: the per-element mean and unbiased standard deviation over the members, (B, C, H, W)
    each, and the quantile maps (Q, B, C, H, W) for up to 8 `quantiles` in [0, 1] (q = 0 and q = 1 are min and max exactly)."""
    members, _, squeeze = _batched(members)
    mean, std, q = hip_ops.ensemble_stats(members, tuple(quantiles), clamp)
    if squeeze:
        mean, std, q = mean[0], std[0], q[:, 0]
    return {"mean": mean, "std": std, "quantiles": q}


def ensemble_scores(members, truth, clamp=None):
    """Per image, as (B,) float64 device tensors: "crps" (mean over the image), "spread" = sqrt(mean variance), "rmse" of the
    ensemble mean and "spread_skill" = sqrt((N + 1) / N) spread / rmse, which is 1 for a calibrated ensemble (Fortin et al.
    2014); and "rank_histogram", the (B, N + 1) int64 counts of the image's elements by the rank of the truth among the members
    (flat for a calibrated ensemble)."""
    members, truth, _ = _batched(members, truth)
    sums, hist, _ = hip_ops.ensemble_scores(members, truth, clamp)
    N, n = members.shape[0], truth[0].numel()
    spread, rmse = torch.sqrt(sums[:, 1] / n), torch.sqrt(sums[:, 2] / n)
    return {"crps": sums[:, 0] / n, "spread": spread, "rmse": rmse, "spread_skill": math.sqrt((N + 1) / N) * spread / rmse,
            "rank_histogram": hist}
