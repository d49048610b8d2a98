"""Colour correction of a super-resolved image against its low-resolution observation.

A diffusion super-resolver drifts radiometrically: band means and large-scale brightness move away from the LR image it was
conditioned on, which band ratios (NDVI) and ERGAS / SAM punish directly.  `color_fix` is the cheap post-process StableSR
ships next to its aggregation sampling: it leaves every reverse chain alone, keeps the sample's fine detail and takes the
large-scale content from `guide`, the LR image brought to the sample's size.  Per (image, band) plane of fp32 ROCm tensors, on
two HIP kernels (csrc/colorfix.hip through `hip_ops.colorfix_wavelet` / `hip_ops.colorfix_adain`; there is no CPU path):

    wavelet   out = (sr - low_L(sr)) + low_L(guide), low_L = blur_{2^(L-1)} o ... o blur_1 with blur_d the 3 x 3 binomial
              kernel (1/4, 1/2, 1/4)^2 of dilation d on replicate padding, L = `levels` in 1 .. 5 (the last blur reaches
              2^L - 1 pixels: L = 5 replaces what is coarser than about 32 pixels)
    adain     out = (sr - mean_sr) / std_sr * std_guide + mean_guide with unbiased variances and std = sqrt(var + 1e-5)

Neither clamps: the tiler and `Diffusion.evaluate` clamp where they did before.
"""
import torch

from . import hip_ops

METHODS = ("wavelet", "adain")
DEFAULT_LEVELS = 5


def check_color_fix_args(method, levels=None):
    """ValueError for a correction `color_fix` cannot run (checked before anything is sampled); returns the levels to use
    (None for adain).  `levels` None: the default."""
    if method not in METHODS:
        raise ValueError(f"color_fix method={method!r} must be one of {METHODS}")
    if method == "adain":
        if levels is not None:
            raise ValueError("levels belongs to method='wavelet': adain has none")
        return None
    levels = DEFAULT_LEVELS if levels is None else levels
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= 5:
        raise ValueError(f"levels must be an integer in 1 .. 5, got {levels!r}")
    return levels


def fix_levels(method, levels=DEFAULT_LEVELS):
    """The `levels` argument of `color_fix` for the (`color_fix`, `color_fix_levels`) pair of the tiler, `Diffusion.evaluate`
    and the command lines, whose level count has the default 5 whatever the method: ValueError as `check_color_fix_args`, and
    for adain with a level count other than that default."""
    if method == "adain" and levels != DEFAULT_LEVELS:
        raise ValueError(f"color_fix_levels={levels!r} belongs to color_fix='wavelet': adain has no levels")
    return check_color_fix_args(method, None if method == "adain" else levels)


def add_color_fix_args(p):
    """--color_fix / --color_fix_levels of the command lines that correct their samples (`cli_color_fix`)."""
    p.add_argument("--color_fix", type=str, choices=("none",) + METHODS, default="none",
                   help="correct the super-resolved output against the up-sampled LR image: wavelet (its large-scale content "
                        "replaced by the LR image's) or adain (per-band mean and deviation matched); default: none")
    p.add_argument("--color_fix_levels", type=int, default=DEFAULT_LEVELS,
                   help="with --color_fix wavelet: the number of dilated blurs, 1 .. 5 (default 5)")
    return p


def cli_color_fix(args):
    """The `color_fix=` / `color_fix_levels=` arguments of a command line; {} without --color_fix (the call is then today's)."""
    method = getattr(args, "color_fix", "none")
    if method in (None, "none"):
        return {}
    return {"color_fix": method, "color_fix_levels": getattr(args, "color_fix_levels", DEFAULT_LEVELS)}


def color_fix(sr, lr=None, *, guide=None, magnification_factor=None, method="wavelet", levels=None):
    """`sr` (B, C, H, W), or one (C, H, W) scene, corrected against exactly one of `lr` - the (B, C, H / m, W / m) observation,
    up-sampled here with `hip_ops.bicubic_upsample` by `magnification_factor` = m - and `guide`, an image of sr's shape.
    `method`: "wavelet" (`levels` 1 .. 5, default 5) or "adain" (takes no `levels`).  Returns a new tensor of sr's shape.
    ValueError: an unknown method, both or neither of lr / guide, a magnification without lr or lr without one, levels
    with adain or outside 1 .. 5, shapes that do not fit."""
    levels = check_color_fix_args(method, levels)
    if (lr is None) == (guide is None):
        raise ValueError("color_fix needs exactly one of lr (with magnification_factor) and guide")
    if (lr is None) != (magnification_factor is None):
        raise ValueError("lr and magnification_factor go together (a guide is already of sr's size)")
    if not isinstance(sr, torch.Tensor) or sr.dim() not in (3, 4):
        raise ValueError("sr must be a (B, C, H, W) or (C, H, W) tensor")
    scene = sr.dim() == 3
    other = lr if lr is not None else guide
    if other.dim() != sr.dim():
        raise ValueError(f"sr {tuple(sr.shape)} and {'lr' if lr is not None else 'guide'} {tuple(other.shape)} must have the "
                         "same number of axes")
    if scene:
        sr, other = sr.unsqueeze(0), other.unsqueeze(0)
    if lr is not None:
        m = int(magnification_factor)
        if m < 1 or (other.shape[0], other.shape[1], other.shape[2] * m, other.shape[3] * m) != tuple(sr.shape):
            raise ValueError(f"lr {tuple(other.shape)} up-sampled by {magnification_factor} is not sr's {tuple(sr.shape)}")
        other = hip_ops.bicubic_upsample(other, m)
    elif other.shape != sr.shape:
        raise ValueError(f"guide {tuple(other.shape)} must have sr's shape {tuple(sr.shape)}")
    sr, other = sr.contiguous(), other.contiguous()
    out = hip_ops.colorfix_wavelet(sr, other, levels) if method == "wavelet" else hip_ops.colorfix_adain(sr, other)
    return out[0] if scene else out
