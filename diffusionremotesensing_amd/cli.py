"""The command-line pieces that the three trainers, `evaluate` and the aggregation tiler share: the reference's common flags,
the sampling flags, and the flags of `Diffusion.train` that are not in the reference (`TRAIN_FLAGS`: one table, from which the
parsers, the defaults and the keyword arguments of `train` are all read)."""
import argparse

from .sampling import sampling_plan


def str2bool(v):
    return v.lower() in ("yes", "true", "t", "1")


def base_arg_parser():
    """The reference's flags that all three trainers have, verbatim (:703-724), and the DDIM flags (`add_sampling_args`)."""
    p = argparse.ArgumentParser(description=" ")
    p.add_argument("--epochs", type=int, default=501)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--image_size", type=int)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--check_preds_epoch", type=int, default=20)
    p.add_argument("--noise_schedule", type=str, default="cosine")
    p.add_argument("--snapshot_name", type=str, default="snapshot.pt")
    p.add_argument("--model_name", type=str)
    p.add_argument("--noise_steps", type=int, default=200)
    p.add_argument("--patience", type=int, default=10)
    p.add_argument("--dataset_path", type=str, default=None)
    p.add_argument("--generate_video", type=str2bool, nargs="?", const=True, default=False)
    p.add_argument("--loss", type=str)
    p.add_argument("--UNet_type", type=str, default="Residual Attention UNet")
    p.add_argument("--multiple_gpus", type=str2bool, nargs="?", const=True, default=False)
    p.add_argument("--ema_smoothing", type=str2bool, nargs="?", const=True, default=False)
    add_sampling_args(p)
    return p


def add_sampling_args(p):
    """The DDIM flags of the final sampling (not in the reference): none = the reference's ancestral chain."""
    p.add_argument("--sampling_steps", type=int, default=None,
                   help="sample with DDIM over this many timesteps (1 .. noise_steps - 1); default: the full ancestral chain")
    p.add_argument("--eta", type=float, default=0.0, help="DDIM eta: 0 deterministic, 1 DDPM-like (with --sampling_steps)")


def add_solver_args(p):
    """--solver / --spacing for the command lines that take them next to --sampling_steps (`cli_sampling_steps`)."""
    p.add_argument("--solver", type=str, choices=("ddim", "dpmpp_2m"), default="ddim",
                   help="how the --sampling_steps steps are taken: ddim, or dpmpp_2m (DPM-Solver++(2M): second order, eta 0)")
    p.add_argument("--spacing", type=str, choices=("uniform", "logsnr"), default=None,
                   help="where the --sampling_steps levels lie: uniform in t or uniform in logSNR; default: uniform for ddim, "
                        "logsnr for dpmpp_2m")
    return p


def cli_sampling_steps(args):
    """The `sampling_steps` argument of a command line: --sampling_steps, as a `sampling_plan` when --solver / --spacing say more."""
    solver, spacing = getattr(args, "solver", "ddim"), getattr(args, "spacing", None)
    steps = getattr(args, "sampling_steps", None)
    return steps if solver == "ddim" and spacing is None else sampling_plan(steps, solver, spacing)


def add_prediction_args(p, in_help=True):
    """--prediction / --x0_clip / --x0_threshold of the outer command lines (the trainers' `main` parsers, `evaluate`, the
    tiler): the `prediction` / `x0_clip` of `Diffusion` (`cli_prediction`) and its `x0_threshold` (`cli_threshold`).  `in_help` False registers them without a --help entry: the
    trainers' help texts are recorded (tests/golden/train_loop_transcripts.json), README.md describes the flags."""
    p.add_argument("--prediction", type=str, choices=("eps", "v", "x0"), default="eps",
                   help="what the network predicts: the noise eps (the reference), v = sqrt(ah) eps - sqrt(1 - ah) x0, or the "
                        "clean image x0; training writes it into the snapshot, which refuses to load as another"
                        if in_help else argparse.SUPPRESS)
    p.add_argument("--x0_clip", type=cli_x0_clip, default=None,
                   help="'none' or 'LO,HI' (--x0_clip=-1,1 for a negative bound): clamp the clean image every reverse step "
                        "implies to this range while sampling; default none" if in_help else argparse.SUPPRESS)
    p.add_argument("--x0_threshold", type=cli_x0_threshold, default=None,
                   help="P, 0 < P <= 1, with --x0_clip: dynamic thresholding (Imagen) - per image, where the P-quantile of "
                        "|x0 - centre| exceeds the half-range, the clean image is compressed into the range instead of clamped; "
                        "default none" if in_help else argparse.SUPPRESS)
    p.add_argument("--zero_terminal_snr", type=str2bool, nargs="?", const=True, default=False,
                   help="rescale the noise schedule to zero terminal SNR (alpha_hat[T-1] = 0; needs --prediction v or x0); "
                        "training writes it into the snapshot, which refuses to load under the other schedule"
                        if in_help else argparse.SUPPRESS)
    p.add_argument("--guidance_rescale", type=cli_guidance_rescale, default=0.0, metavar="PHI",
                   help="PHI in [0, 1]: rescale the classifier-free-guided prediction per image towards the standard deviation "
                        "of the conditional one (acts where a sampler guides with cfg_scale > 0); default 0"
                        if in_help else argparse.SUPPRESS)
    return p


def cli_guidance_rescale(text):
    """The value of --guidance_rescale: a PHI in [0, 1], read while the command line is parsed."""
    try:
        phi = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be a number in [0, 1]") from None
    if not 0.0 <= phi <= 1.0:
        raise argparse.ArgumentTypeError(f"{text!r} must lie in [0, 1]")
    return phi


def cli_ztsnr(args):
    """`add_prediction_args`' --zero_terminal_snr as a keyword argument of a `Diffusion` (merged next to `cli_prediction`; a
    namespace without it: off)."""
    return {"zero_terminal_snr": bool(getattr(args, "zero_terminal_snr", False))}


def set_guidance_rescale(diffusion, args):
    """`add_prediction_args`' --guidance_rescale onto a `Diffusion` (a plain attribute; a namespace without it: 0); returns it."""
    diffusion.guidance_rescale = float(getattr(args, "guidance_rescale", 0.0) or 0.0)
    return diffusion


def cli_x0_threshold(text):
    """The value of --x0_threshold as `Diffusion`'s `x0_threshold`: a P in (0, 1], read while the command line is parsed."""
    try:
        p = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be a number in (0, 1]") from None
    if not 0.0 < p <= 1.0:
        raise argparse.ArgumentTypeError(f"{text!r} must lie in (0, 1]")
    return p


def cli_x0_clip(text):
    """The value of --x0_clip as `Diffusion`'s `x0_clip`: None for 'none', (LO, HI) for 'LO,HI' - the words of the tiler's
    --clamp (`Aggregation_Sampling.cli_clamp`), read while the command line is parsed, so that a bad value ends every parser."""
    if text.strip().lower() == "none":
        return None
    try:
        lo, hi = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be 'none' or 'LO,HI'") from None
    if not lo < hi:
        raise argparse.ArgumentTypeError(f"{text!r} needs LO < HI")
    return lo, hi


def cli_prediction(args):
    """`add_prediction_args`' flags as keyword arguments of a `Diffusion` (a namespace without them: the defaults)."""
    return {"prediction": getattr(args, "prediction", "eps"), "x0_clip": getattr(args, "x0_clip", None)}


def cli_threshold(args):
    """`add_prediction_args`' --x0_threshold as a keyword argument of a `Diffusion` (merged next to `cli_prediction`; a
    namespace without it: off).  Without --x0_clip the constructor refuses it (`sampling.check_threshold`)."""
    return {"x0_threshold": getattr(args, "x0_threshold", None)}


def cli_nonnegative(text):
    """The value of --lr_damping / --lr_blur_radius: a finite number >= 0, read while the command line is parsed."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be a number >= 0") from None
    if not 0.0 <= v < float("inf"):
        raise argparse.ArgumentTypeError(f"{text!r} must be a finite number >= 0")
    return v


def cli_finite(text):
    """The value of --lr_strength: a finite number."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be a finite number") from None
    if not abs(v) < float("inf"):
        raise argparse.ArgumentTypeError(f"{text!r} must be a finite number")
    return v


def add_consistency_args(p):
    """--lr_consistency and --lr_damping / --lr_strength / --lr_blur_radius of `evaluate` (superres) and the tiler
    (`cli_consistency`; consistency.py).  Not in the reference, and not on the trainers."""
    p.add_argument("--lr_consistency", type=str2bool, nargs="?", const=True, default=False,
                   help="LR-consistent sampling: project the clean image every reverse step implies (the tiler: also the finished "
                        "scene) onto the images the degradation maps to the LR input; needs --Degradation_type DownBlur or "
                        "DownBlurNoise, or an MTF run (--mtf_nyquist: each band's own operator)")
    p.add_argument("--lr_damping", type=cli_nonnegative, default=0.01, metavar="D",
                   help="with --lr_consistency: the Tikhonov damping of the projection's gain (0: the exact pseudo-inverse, "
                        "refused for an ill-conditioned blur); default 0.01")
    p.add_argument("--lr_strength", type=cli_finite, default=1.0, metavar="S",
                   help="with --lr_consistency: the share of the correction that is applied; default 1")
    p.add_argument("--lr_blur_radius", type=cli_nonnegative, default=None, metavar="R",
                   help="with --lr_consistency: the blur radius of the degradation the LR input was made with; default: the "
                        "trainer's 0.5")
    return p


def cli_consistency(args):
    """`add_consistency_args`' flags as the `lr_consistency` keyword of `Diffusion.evaluate` and the tiler's
    `aggregation_sampling`: None without --lr_consistency (and for a namespace without the flags), else an `LRConsistency`.
    ValueError for --lr_damping / --lr_strength / --lr_blur_radius without it."""
    given = [name for name, default in (("lr_damping", 0.01), ("lr_strength", 1.0), ("lr_blur_radius", None))
             if getattr(args, name, default) != default]
    if not getattr(args, "lr_consistency", False):
        if given:
            raise ValueError("--" + " / --".join(given) + " belong to --lr_consistency")
        return {"lr_consistency": None}
    from .consistency import LRConsistency
    return {"lr_consistency": LRConsistency(blur_radius=getattr(args, "lr_blur_radius", None),
                                            damping=getattr(args, "lr_damping", 0.01),
                                            strength=getattr(args, "lr_strength", 1.0))}


def cli_prefixes(text):
    """The value of --freeze: 'PREFIX[,PREFIX...]' as a tuple of state_dict-key prefixes (empty pieces: an error)."""
    parts = tuple(s.strip() for s in text.split(","))
    if not all(parts):
        raise argparse.ArgumentTypeError(f"{text!r} must be PREFIX[,PREFIX...] of state_dict keys, e.g. downs.,LR_encoder.")
    return parts


def add_finetune_args(p):
    """--freeze_bn / --freeze / --init_from of the trainers' `main` parsers: `Diffusion.train`'s `freeze_bn`, `freeze` and
    `init_from` (`cli_finetune`; finetune.py).  Registered without a --help entry, like
    `add_prediction_args(in_help=False)`: the trainers' help texts are recorded, README.md describes the flags."""
    p.add_argument("--freeze_bn", type=str2bool, nargs="?", const=True, default=False, help=argparse.SUPPRESS)
    p.add_argument("--freeze", type=cli_prefixes, default=(), help=argparse.SUPPRESS)
    p.add_argument("--init_from", type=str, default=None, help=argparse.SUPPRESS)
    return p


def cli_finetune(args):
    """`add_finetune_args`' flags as keyword arguments of `Diffusion.train` (a namespace without them: the defaults)."""
    return {"freeze_bn": bool(getattr(args, "freeze_bn", False)), "freeze": tuple(getattr(args, "freeze", ()) or ()),
            "init_from": getattr(args, "init_from", None)}


def cli_nodata(text):
    """The value of the SAR -> NDVI trainer's and `evaluate`'s --nodata: 'nan' (a pixel with a NaN band is no-data) or the
    no-data value V (also a pixel whose bands all equal V), read while the command line is parsed."""
    if text.strip().lower() == "nan":
        return "nan"
    try:
        value = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be 'nan' or a number") from None
    if value != value:
        return "nan"
    if value in (float("inf"), float("-inf")):
        raise argparse.ArgumentTypeError(f"{text!r} must be finite")
    return value


def cli_nodata_u8(text):
    """The value of the super-resolution trainer's --nodata: an integer K in 0 .. 255, the stored pixel value that marks no-data."""
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be an integer in 0 .. 255") from None
    if not 0 <= k <= 255:
        raise argparse.ArgumentTypeError(f"{text!r} must lie in 0 .. 255")
    return k


def cli_nodata_u16(text):
    """--nodata of a super-resolution command line that also has --bit_depth: an integer K in 0 .. 65535; `check_nodata_depth`
    holds it to 0 .. 255 once the bit depth is known."""
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} must be an integer in 0 .. 255") from None
    if not 0 <= k <= 65535:
        raise argparse.ArgumentTypeError(f"{text!r} must lie in 0 .. 255" if k < 0 else f"{text!r} must lie in 0 .. 65535")
    return k


def check_nodata_depth(p, args):
    """`p.error`, in `cli_nodata_u8`'s words, for a --nodata above 255 without --bit_depth 16."""
    k = getattr(args, "nodata", None)
    if k is not None and k > 255 and int(getattr(args, "bit_depth", 8) or 8) != 16:
        p.error(f"argument --nodata: {str(k)!r} must lie in 0 .. 255")
    return args


def add_nodata_args(p, in_help=True, u8=False):
    """--nodata of the two conditional trainers and `evaluate`.  `u8`: the super-resolution form, an
    integer pixel value K (the rule value is float32(K) / 255, the bits the u8 feeds produce); otherwise 'nan' or a number.
    `in_help` False registers it without a --help entry, as `add_prediction_args` does for the trainers."""
    text = ("K in 0 .. 255: HR pixels whose bands all hold K are no-data - left out of the loss and the scores (DownBlur only; "
            "the LR image is still made from the stored pixels)" if u8 else
            "'nan' or V: pixels of the truth with a NaN band (and, with V, whose bands all equal V) are no-data - left out of "
            "the loss and the scores")
    p.add_argument("--nodata", type=cli_nodata_u8 if u8 else cli_nodata, default=None, help=text if in_help else argparse.SUPPRESS)
    return p


def add_bsr_args(p):
    """--bsr_kind / --bsr_seed of the command lines that build the BSRGAN feed (not in the reference; `make_superres_feeds`)."""
    p.add_argument("--bsr_kind", type=str, choices=("plus", "soft"), default="plus",
                   help="with --Degradation_type BSRGAN: plus (degradation_bsrgan_plus: USM, two rounds of blur / resize / noise, "
                        "JPEG) or soft (blur, resize, noise once)")
    p.add_argument("--bsr_seed", type=int, default=0, help="with --Degradation_type BSRGAN: seed of the recipes and the noise")
    return p


# -- the flags of `Diffusion.train` that are not in the reference ----------------------------------------------------------------
# {group: {keyword of `train`: the `add_argument` keywords of --<keyword>}}, in the order --help lists them.  A new group is a new
# entry here and, if its values need checking, in `check_train_args`.
TRAIN_FLAGS = {
    "optim": {  # optimizer / schedule / resume (optim.py)
        "weight_decay": dict(type=float, default=0.0, help="decoupled (AdamW) weight decay; 0 = the reference's Adam"),
        "max_grad_norm": dict(type=float, default=None,
                              help="clip the global gradient norm to this value; steps with non-finite gradients are skipped"),
        "lr_schedule": dict(type=str, choices=("constant", "cosine"), default="constant",
                            help="after --warmup_steps: stay at --lr, or half a cosine down to --lr_min at the last step"),
        "warmup_steps": dict(type=int, default=0, help="optimizer steps of linear learning-rate warm-up"),
        "lr_min": dict(type=float, default=0.0, help="final learning rate of --lr_schedule cosine"),
        "save_train_state": dict(
            type=str2bool, nargs="?", const=True, default=False,
            help="write train_state.pt (optimizer, raw weights under EMA, schedule, early-stopping and RNG state) beside "
                 "every snapshot, and continue from both when they exist.  Not built: gradient accumulation, loss scaling, "
                 "the crop / BSRGAN feeds' own generators, per-rank files (rank 0 writes, every rank reads)"),
    },
    "objective": {  # the training objective (losses.py)
        "loss_weighting": dict(type=str, choices=("none", "min_snr"), default="none",
                               help="min_snr: weight every image's loss with min(1, --min_snr_gamma / SNR_t); none = the "
                                    "reference's loss"),
        "min_snr_gamma": dict(type=float, default=5.0, help="gamma of --loss_weighting min_snr"),
        "timestep_sampling": dict(
            type=str, choices=("uniform", "loss_aware"), default="uniform",
            help="loss_aware: draw t on the device in proportion to the recent losses of its timestep bin, with the "
                 "importance weight that keeps the loss an estimate of the uniform mean; uses 16 bins when --loss_bins "
                 "is 0 and consumes the device generator instead of the CPU one"),
        "loss_bins": dict(type=int, default=0,
                          help="keep and print the mean loss per timestep bin (N bins, 2 .. 64 and at most noise_steps / 2; "
                               "lowest-noise bin first), one more line per phase and epoch; 0 = off.  Not built: bins shared "
                               "across ranks, weighting of the perceptual loss"),
    },
}
OPTIM_DEFAULTS = {k: kw["default"] for k, kw in TRAIN_FLAGS["optim"].items()}
OBJECTIVE_DEFAULTS = {k: kw["default"] for k, kw in TRAIN_FLAGS["objective"].items()}


def _add_group(p, group):
    for name, kw in TRAIN_FLAGS[group].items():
        p.add_argument("--" + name, **kw)
    return p


def add_optim_args(p):
    return _add_group(p, "optim")


def add_objective_args(p):
    return _add_group(p, "objective")


def add_train_args(p):
    """Every group of `TRAIN_FLAGS` on the parser of a trainer's command line."""
    for group in TRAIN_FLAGS:
        _add_group(p, group)
    return p


def check_optim_args(p, args):
    if args.weight_decay < 0 or args.lr_min < 0 or args.warmup_steps < 0:
        p.error("--weight_decay, --lr_min and --warmup_steps must be >= 0")
    if args.max_grad_norm is not None and not args.max_grad_norm > 0:
        p.error("--max_grad_norm must be > 0")
    return args


def check_objective_args(p, args):
    if args.loss_bins < 0 or not args.min_snr_gamma > 0:
        p.error("--loss_bins must be >= 0 and --min_snr_gamma > 0")
    return args


def check_train_args(p, args):
    """`p.error` for a value of `add_train_args`' flags that no run takes; returns `args`."""
    check_optim_args(p, args)
    return check_objective_args(p, args)


def optim_train_kwargs(args):
    return {k: getattr(args, k, v) for k, v in OPTIM_DEFAULTS.items()}


def objective_train_kwargs(args):
    return {k: getattr(args, k, v) for k, v in OBJECTIVE_DEFAULTS.items()}


def train_kwargs(args):
    """`add_train_args`' flags as keyword arguments of `Diffusion.train` (a namespace without them: the defaults)."""
    return {**optim_train_kwargs(args), **objective_train_kwargs(args)}
