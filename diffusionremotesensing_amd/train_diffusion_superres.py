"""Drop-in `Diffusion` (schedules, q-sample, ancestral sampler, training loop, snapshots),
`launch(args)` and the CLI of reference train_diffusion_superres.py, with the arithmetic on
the gfx950 kernels of include/drs_hip.h.

Kept verbatim from the reference: constructor signature and attributes (:79-126), method names,
the snapshot file format {"MODEL_STATE", "EPOCHS_RUN"} (:257-308) and the 21 CLI flags (:703-724).
Deliberately different (documented in DESIGN.md):
  * `from_alpha_hat_to_beta` is vectorised (same fp32 operations, bit-identical values) instead of a
    T-iteration Python loop (:143-148);
  * `sample` computes the LR-conditioning branch once per chain and updates x with one fused kernel;
    the per-step timestep tensor lives on the device instead of being rebuilt on the host (:235);
  * multi-GPU uses one flat-buffer RCCL all-reduce per step (`dist.allreduce_gradients`) instead of
    DistributedDataParallel(find_unused_parameters=True) (:658).

`Diffusion.train` is an epoch loop over named steps that share one `TrainRun` (`Diffusion.train_state`).  What the reference
keeps in this file besides the class lives next to it and is re-exported here under its old names: the flag helpers in cli.py,
the launcher pieces the three trainers share in launcher.py, the dataset and the feeds in superres_feeds.py.
"""
import copy
import os
import types

import torch
import torch.nn as nn

from . import dist as drs_dist
from . import hip_ops
from . import mtf
from . import radiometry
from .augment import add_augment_args
# (the names this module does not use itself are re-exported: they lived here before cli.py, launcher.py and superres_feeds.py)
from .cli import (OBJECTIVE_DEFAULTS, OPTIM_DEFAULTS, add_bsr_args, add_finetune_args, add_nodata_args, add_objective_args, add_optim_args, check_nodata_depth, cli_nodata_u16,  # noqa: F401
                  add_prediction_args, add_sampling_args, add_solver_args, add_train_args, base_arg_parser, check_objective_args, check_optim_args,
                  check_train_args, cli_sampling_steps, objective_train_kwargs, optim_train_kwargs, str2bool)
from .finetune import freeze_parameters, load_init_weights
from .launcher import launch_device, make_loaders, save_final_samples, train_model  # noqa: F401
from .losses import DiffusionLoss, LossAwareSampler, LossBins, min_snr_weights
from .optim import FusedAdam, FusedAdamW, WarmupCosine
from .sampling import (CHAIN_CHECK_EVERY, _is_int, _repeat_members, asks_for_known_pixels,  # noqa: F401 - re-exported
                       check_ensemble_args, check_inpaint_args, check_prediction, check_sampling_args, check_threshold, check_solver_known,
                       check_chain_consistency, check_terminal_chain, check_zero_terminal_snr, ddim_chain_noise,
                       rescale_zero_terminal_snr, ddim_timesteps, ensemble_chunks, inpaint_schedule, known_tensors, run_reverse_chain, sample_chain,
                       sampling_plan)
from .superres_feeds import SyntheticSuperresDataset, make_superres_feeds  # noqa: F401
from .UNet_model_superres import EMA, Residual_Attention_UNet_superres

_DEGRADATIONS = ("downblur", "bsrgan", "downblurnoise", "mtf")

METRIC_FORMATS = {"psnr": ("PSNR", "{:.2f} dB"), "ssim": ("SSIM", "{:.4f}"), "sam": ("SAM", "{:.3f} deg"),
                  "ergas": ("ERGAS", "{:.4g}"), "psnr_unknown": ("PSNR unknown", "{:.2f} dB"),
                  "valid_fraction": ("valid", "{:.4f}"), "lr_rmse": ("LR RMSE", "{:.4g}")}


def format_scores(scores):
    """One line of `Diffusion.evaluate`'s means: PSNR to 0.01 dB, SSIM to 4 decimals, SAM to 0.001 degrees, ERGAS to 4
    significant digits, the model's figures and - where scored - the colour-corrected model's and the bicubic baseline's."""
    parts = []
    for name in ("model", "model_fixed", "bicubic"):
        if name in scores:
            parts.append(name + " " + " ".join(f"{METRIC_FORMATS[k][0]} {METRIC_FORMATS[k][1].format(v)}"
                                               for k, v in scores[name].items()))
    return " | ".join(parts)


class TrainRun:
    """What one `Diffusion.train` call holds besides the weights, kept as `Diffusion.train_state` (`Diffusion._begin_run` makes
    it): the parts `train_step` is called with, the objective behind `loss_function` (None for a default run: then it is torch's
    module), the flags that steer the loop, and early stopping's two counters - the only copy of them, which `train_state.pt`
    is written from and read into."""

    def __init__(self, model, loss, optimizer, scheduler, ema, ema_model, objective, loss_function, clipping, save_train_state):
        self.model, self.loss = model, loss  # the network that is trained; the loss's name in the report lines
        self.optimizer, self.scheduler, self.ema, self.ema_model = optimizer, scheduler, ema, ema_model
        self.saved = ema_model if ema_model is not None else model  # the network that is validated, scored and snapshotted
        self.objective, self.loss_function = objective, loss_function
        self.loss_bins = objective.bins if objective is not None else None
        self.clipping, self.save_train_state = clipping, save_train_state
        self.best_loss, self.epochs_without_improving = float("inf"), 0
        self.skipped_before = 0  # the optimizer's count of skipped steps at the end of the last epoch (it is new: none yet)


class Diffusion:
    def __init__(self, noise_schedule: str, model: nn.Module, snapshot_path: str, noise_steps=1000, beta_start=1e-4,
                 beta_end=0.02, device="cuda", magnification_factor=4, image_size=224, model_name="superres",
                 Degradation_type="BSRGAN", multiple_gpus=False, ema_smoothing=False, prediction="eps", x0_clip=None,
                 x0_threshold=None, zero_terminal_snr=False, mtf_nyquist=None, mtf_noise=None):
        # not in the reference, whose networks predict the noise: what this one predicts ("eps", "v" or "x0": the training
        # target, and what sampling converts to eps before every update) and the range the x0 implied at every reverse step
        # is clamped to (None or (lo, hi); a plain attribute, read at the start of every chain).  DESIGN.md section 23.
        self.prediction, self.x0_clip = check_prediction(prediction, x0_clip)
        # ... and the quantile of dynamic thresholding (None, or p in (0, 1] with an x0_clip: per image, where the p-quantile of
        # |x0 - centre| exceeds the half-range, x0 is compressed into the range instead of cut off at it).  A plain attribute
        # like x0_clip, not written into snapshots.  DESIGN.md section 24.
        self.x0_threshold = check_threshold(x0_threshold, self.x0_clip)
        # ... and a schedule rescaled to zero terminal SNR (alpha_hat[T - 1] == 0: the network is trained on pure noise at the
        # level every sampler starts from; needs a v or x0 network, written into snapshots), with the guidance rescale that goes
        # with it (phi in [0, 1], a plain attribute; acts where a sampler guides with cfg_scale > 0).  DESIGN.md section 26.
        self.zero_terminal_snr = check_zero_terminal_snr(zero_terminal_snr, self.prediction)
        self.guidance_rescale = 0.0
        # ... and the no-data marker of the clean images (None: every pixel is data; True: a pixel with a NaN band is no-data;
        # a number: also a pixel whose bands all equal it).  A plain attribute, read by `_noised_target`, the train and validation
        # steps and `train`'s --eval_metrics scores; `nodata_fill` is what the network sees under the mask, forward-noised.
        # DESIGN.md section 27.
        self.nodata, self.nodata_fill = None, 0.5
        # ... and LR-consistent sampling (None, or a consistency.LRConsistency: every reverse move of `sample` projects the x0 it
        # implies onto the images the degradation maps to the LR image, with the DownBlur operator of `blur_radius` unless the
        # request names another).  Plain attributes like x0_clip, read at the start of every chain, not written into snapshots;
        # the super-resolution sampler only.  DESIGN.md section 28.
        self.lr_consistency, self.blur_radius = None, 0.5
        # ... and the band ranges of a 16-bit run (None, or the (C, 2) fp32 table (lo_c, hi_c) the uint16 feed normalises with:
        # radiometry.py).  A plain attribute: written into snapshots and train_state.pt when set, and
        # `snapshot_data_range` is what the loaded snapshot holds (None: an 8-bit run's file).
        self.data_range, self.snapshot_data_range = None, None
        self.noise_steps = noise_steps
        self.beta_start = beta_start
        self.beta_end = beta_end
        self.image_size = image_size
        self.model_name = model_name
        self.magnification_factor = magnification_factor
        self.device = device
        self.snapshot_path = snapshot_path
        self.Degradation_type = Degradation_type
        # ... and the sensor-MTF degradation (Degradation_type "MTF": mtf.py): per band, the gain of the
        # Gaussian blur at the LR Nyquist frequency and the standard deviation of the sensor noise, tuples of C floats (a number
        # or "G1,..,GC" is spread / parsed; both None for every other degradation).  `mtf_nyquist` is written into snapshots and
        # train_state.pt of an MTF run - no other run writes the key - and a file written under other gains is refused.
        self.mtf_nyquist, self.mtf_noise = self._check_mtf(Degradation_type, mtf_nyquist, mtf_noise, model, magnification_factor)
        self.multiple_gpus = multiple_gpus
        self.ema_smoothing = ema_smoothing
        self.model = model.to(self.device)
        self.epochs_run = 0
        self.timestep_sampler = None  # `train(timestep_sampling="loss_aware")` puts a losses.LossAwareSampler here
        if os.path.exists(snapshot_path):
            print("Loading snapshot")
            self._load_snapshot()

        self.noise_schedule = noise_schedule
        if noise_schedule == "linear":
            self.beta = self.prepare_noise_schedule().to(self.device)
            self.alpha = 1.0 - self.beta
            self.alpha_hat = torch.cumprod(self.alpha, dim=0)
        elif noise_schedule == "cosine":
            self.alpha_hat = self.prepare_noise_schedule().to(self.device)
            self.beta = self.from_alpha_hat_to_beta()
            self.alpha = 1.0 - self.beta
        # any other name leaves the schedule unset, like the reference (:117-126)
        if self.zero_terminal_snr and noise_schedule in ("linear", "cosine"):
            self.alpha_hat = rescale_zero_terminal_snr(self.alpha_hat)
            self.beta = self.from_alpha_hat_to_beta()  # (beta[T - 1] == 1, alpha[T - 1] == 0)
            self.alpha = 1.0 - self.beta

    # -- schedules (reference :128-169) ---------------------------------------------------------
    def prepare_noise_schedule(self):
        if self.noise_schedule == "linear":
            return torch.linspace(self.beta_start, self.beta_end, self.noise_steps)
        elif self.noise_schedule == "cosine":
            steps = torch.arange(self.noise_steps) / self.noise_steps
            f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
            return f_t / f_t[0]

    def from_alpha_hat_to_beta(self):
        ah = self.alpha_hat
        beta = torch.empty_like(ah)
        beta[0] = 1 - ah[0]
        beta[1:] = 1 - ah[1:] / ah[:-1]
        return beta

    # -- forward process (reference :171-205) ---------------------------------------------------
    def noise_images(self, x, t):
        epsilon = torch.randn_like(x, dtype=torch.float32)
        return hip_ops.noise_images(x, epsilon, t, self.alpha_hat), epsilon

    def sample_timesteps(self, n):
        return torch.randint(low=1, high=self.noise_steps, size=(n,))

    def _noised_target(self, x0, t):
        """(x_t, what the network is trained to return for it) of a clean batch at the levels t, for the training and the
        validation loop alike: `noise_images`' pair for "eps"; its x_t and the clean batch for "x0"; for "v" the same draw
        of eps, x_t and v from one launch (`hip_ops.noise_v_target`: that x_t is `noise_images`').  With `self.nodata` set the
        mask comes back as well, (x_t, target, valid) from one launch (`hip_ops.noise_target_nodata`): at valid pixels the same
        bits, at no-data pixels the noised `nodata_fill` and a target of 0."""
        if self.nodata is not None:
            epsilon = torch.randn_like(x0, dtype=torch.float32)
            return hip_ops.noise_target_nodata(x0, epsilon, t, self.alpha_hat, self.prediction, self.nodata, self.nodata_fill)
        if self.prediction == "v":
            epsilon = torch.randn_like(x0, dtype=torch.float32)
            return hip_ops.noise_v_target(x0, epsilon, t, self.alpha_hat)
        x_t, noise = self.noise_images(x0, t)
        return x_t, (x0 if self.prediction == "x0" else noise)

    def _noised(self, x0, t):
        """`_noised_target` as the two loops take it: always (x_t, target, valid), `valid` None for a run without `nodata`."""
        out = self._noised_target(x0, t)
        return out if len(out) == 3 else (*out, None)

    # -- reverse process (reference :207-255) ---------------------------------------------------
    def sample(self, n, model, lr_img, input_channels=3, generate_video=False, noise_source=None, sampling_steps=None,
               eta=0.0):
        """`noise_source(i, shape)`, when given, supplies x_T (i == noise_steps) and the per-step noise z_i
        instead of torch.randn — used to drive this sampler and the oracle with identical noise.
        `sampling_steps=S` runs a DDIM chain over the S timesteps of `ddim_timesteps` instead of the reference's ancestral
        chain (None); `eta` moves it from deterministic (0) to DDPM-like (1) sampling.  (`sample_known` keeps given pixels.)
        `sampling_steps=sampling_plan(S, solver="dpmpp_2m")` takes the S steps with DPM-Solver++(2M) instead - second order, one
        forward per step like DDIM, deterministic (eta = 0) - on logSNR-spaced levels; `sampling_plan(S, spacing="logsnr")` is
        DDIM on those levels (`sampling.sampling_plan`).  Whatever takes `sampling_steps` takes such a plan."""
        return self._sample(n, model, lr_img, input_channels, generate_video, noise_source, sampling_steps, eta)

    def sample_known(self, n, model, lr_img, known, known_mask, input_channels=3, resample=1, jump=1, generate_video=False,
                     noise_source=None, sampling_steps=None, eta=0.0):
        """`sample` with known pixels (RePaint): `known` (C, S, S) or (n, C, S, S), in the model's data range and used as
        given, with `known_mask` (S, S), (1 | C, S, S) or (n, 1 | C, S, S) (bool, uint8 or {0, 1} float; nonzero = known) -
        those pixels are kept and the others sampled.  `resample` and `jump` are its resampling (`inpaint_schedule`; 1 =
        none); everything else is `sample`'s.  See `_sample_chain` for the moves and the noise draws."""
        asks_for_known_pixels(known, known_mask, resample, jump, required=True)
        return self._sample(n, model, lr_img, input_channels, generate_video, noise_source, sampling_steps, eta, known,
                            known_mask, resample, jump)

    def sample_ensemble(self, n_members, model, lr_img, input_channels=3, member_batch=None, sampling_steps=None, eta=0.0,
                        noise_source=None, known=None, known_mask=None, resample=1, jump=1):
        """`n_members` >= 2 samples per LR image: (n_members, B, C, S, S), un-clamped like `sample`, for `lr_img` (B, C, h, w)
        or one (C, h, w) image (B = 1) - the input of `ensemble.ensemble_statistics` / `ensemble.ensemble_scores`.
        The members are drawn `member_batch` at a time (None: all at once; `ensemble_chunks`): every chunk of m members is one
        ordinary `sample` call with m * B chains, member-major, on the LR batch repeated m times, so memory is bounded by the
        chunk and `noise_source` is asked chunk after chunk.  With `known` / `known_mask` ((C, S, S) / (S, S) for every chain,
        or one per image: (B, C, S, S) / (B, 1 | C, S, S)) every chunk is a `sample_known` call instead and all members keep
        those pixels; `resample` / `jump` as there.  `sampling_steps` / `eta` as in `sample`."""
        lr = lr_img if lr_img.dim() == 4 else lr_img.unsqueeze(0)
        args = {"input_channels": input_channels, "noise_source": noise_source, "sampling_steps": sampling_steps, "eta": eta}
        return self._sample_members(n_members, member_batch, lr.shape[0], lambda m: self._ensemble_chunk(
            m * lr.shape[0], (model, lr.repeat(m, 1, 1, 1)), _repeat_members(known, m), _repeat_members(known_mask, m), resample,
            jump, args))

    def _ensemble_chunk(self, n, head, known, known_mask, resample, jump, args):
        """One chunk of `sample_ensemble`: `sample(n, *head, **args)`, or `sample_known` when known pixels are asked for."""
        if not asks_for_known_pixels(known, known_mask, resample, jump):
            return self.sample(n, *head, **args)
        return self.sample_known(n, *head, known, known_mask, resample=resample, jump=jump, **args)

    @staticmethod
    def _sample_members(n_members, member_batch, B, draw):
        """(n_members, B, C, S, S) from `draw(m)` -> the (m * B, C, S, S) chains of m members, chunk after chunk."""
        check_ensemble_args(n_members, member_batch)
        x = torch.cat([draw(m) for m in ensemble_chunks(n_members, member_batch)])
        return x.view(int(n_members), B, *x.shape[1:])

    def _sample(self, n, model, lr_img, input_channels, generate_video, noise_source, sampling_steps, eta, known=None,
                known_mask=None, resample=1, jump=1):
        check_sampling_args(self.noise_steps, sampling_steps, eta)
        check_inpaint_args((n, input_channels, self.image_size, self.image_size), known, known_mask, resample, jump)
        if self.Degradation_type.lower() not in _DEGRADATIONS:
            raise ValueError("The degradation type must be either BSRGAN or DownBlur")
        if lr_img.dim() == 4:
            # extension used by the aggregation tiler: one LR image per chain, (n, C, h, w); the reference only takes a
            # single (C, h, w) image broadcast over the n chains (:224)
            if lr_img.shape[0] != n:
                raise RuntimeError(f"sample: a batch of {lr_img.shape[0]} LR images for n={n} chains")
            lr_img = lr_img.to(self.device).contiguous()
        else:
            lr_img = lr_img.to(self.device).unsqueeze(0).contiguous()
        return self._sample_chain(
            model, (n, input_channels, self.image_size, self.image_size),
            lambda engine, x, t, first: engine.forward(x, t, lr_img, self.magnification_factor, reuse_cond=not first,
                                                       check_weights=first),
            table_rows=n, generate_video=generate_video, noise_source=noise_source, sampling_steps=sampling_steps, eta=eta,
            known=known, known_mask=known_mask, resample=resample, jump=jump, lr_img=lr_img)

    def _sample_chain(self, model, shape, predict, *, table_rows, generate_video, noise_source, sampling_steps, eta,
                      cfg_scale=0.0, update=None, known=None, known_mask=None, resample=1, jump=1, lr_img=None):
        """The reverse chain all three samplers share (reference :226-255), from x_T to the returned x_0.
        `predict(engine, x, t, first)` is the sampler's model call for one step: x in its current state, t one row of the
        (noise_steps, table_rows) timestep table, `first` True on the first call of the chain only (weights checked,
        conditioning branch computed; not set again after a range-fault rollback).  It returns eps, or (eps_cond, eps_uncond)
        for classifier-free guidance: torch.lerp(eps_uncond, eps_cond, cfg_scale) is then folded into the update kernel.
        `update(x, eps, noise, i, i_prev)`, when given, takes the step in place of the sampler / DDIM update kernels (i_prev
        None on the ancestral chain): the tiler's per-step blend, whose state is a scene and whose eps a stack of tiles.
        With `known` / `known_mask` (checked by `check_inpaint_args`) a reverse move t -> t_prev is one `inpaint_step_` (the
        known pixels become `known` forward-noised to t_prev, the others take the sampler's step) and draws one noise tensor -
        `noise_source(t, shape)` - iff t_prev > 0, whatever eta is; a forward jump of `inpaint_schedule` to level t is one
        `renoise_` and draws `noise_source(t, shape)`.  On the ancestral chain without resampling these are the draws of the
        plain sampler.  With an `update` hook as well (the tiler's scene with known pixels) the moves are the same and a
        reverse move calls `update(x, eps, noise, i, i_prev, known=, known_mask=)` with the converted tensors and that draw; a
        forward jump is the `renoise_` of the scene state.  With a `sampling_plan` of solver "dpmpp_2m" the moves are `dpm_step_`s and the `update` hook also gets
        `hist=` and `t_q=`, as `sampling.sample_chain` says.  `lr_img` is the observation `self.lr_consistency` projects onto
        (only `sample` and its relatives here pass one: with the attribute set, a chain without it, or with `update`, raises).
        The chain is `sampling.sample_chain`; this method adds the eval
        mode around it and the video."""
        check_solver_known(sampling_steps, known, known_mask)
        check_terminal_chain(self, self.prediction, eta, update)
        check_chain_consistency(self, update, lr_img, needs_lr=True)
        model.eval()
        frames = [] if generate_video else None
        x = sample_chain(self, self._engine_net(model).hip_engine(), shape, predict, table_rows=table_rows, noise_source=noise_source,
                         sampling_steps=sampling_steps, eta=eta, cfg_scale=cfg_scale, update=update, known=known,
                         known_mask=known_mask, resample=resample, jump=jump, frames=frames, lr_img=lr_img)
        if generate_video:
            from .video import video_maker  # optional dependency (cv2), same call as reference :253
            video_maker(frames, os.path.join(os.getcwd(), "models_run", self.model_name, "results",
                                             "video_denoising.mp4"), 100)
        model.train()  # reference side effect (:254)
        return x

    # -- image quality of the samples (metrics.py; not in the reference) ---------------------------
    def evaluate(self, model, loader, n_images=None, sampling_steps=None, eta=0.0, noise_source=None, baseline=True,
                 known_mask_fn=None, resample=1, jump=1, ensemble=None, member_batch=None, color_fix=None, color_fix_levels=5,
                 lr_consistency=None, nodata=None):
        """PSNR / SSIM / SAM / ERGAS (metrics.image_quality) of `sample`'s output against the ground truth over the (lr, hr)
        batches of `loader`, every batch sampled as one call with n = its size, until `n_images` images are scored (None: the
        whole loader).  `sampling_steps`, `eta` and `noise_source` are `sample`'s (the source is asked batch after batch).
        With `baseline` the bicubic up-sampling of lr is scored next to the model.  `known_mask_fn(truth) -> (n, 1 | C, S, S)`
        mask, when given, samples every batch with its truth as `known` under that mask (`resample` / `jump` as in `sample`)
        and adds "psnr_unknown", the PSNR over the hidden pixels alone (metrics.psnr_masked).  Returns
        {"model": {metric: mean}, "bicubic": {metric: mean}, "per_image": {"model": {metric: [...]}, "bicubic": ...}, "n": N}.
        `ensemble=N` draws N members per image (`sample_ensemble`, `member_batch` as there) instead of one sample: "model"
        then scores the ensemble MEAN, "member" member 0 - the single-draw figure reported without `ensemble` - and
        "ensemble" holds the means of `ensemble.ensemble_scores` (crps, spread, rmse, spread_skill) and the summed
        "rank_histogram", everything on members and truth clamped to [0, 1] like the image scores; see `_evaluate`.
        `color_fix` ("wavelet" with `color_fix_levels`, or "adain"; not with `ensemble` or `known_mask_fn`) adds a third
        estimate, "model_fixed": the very sample "model" scored - each batch is still sampled once - clamped to [0, 1] as
        the scores clamp it and corrected against the bicubic up-sampling of its lr batch (`colorfix.color_fix`).
        `nodata` (True / "nan" or the no-data value; not with `ensemble` or `known_mask_fn`) scores every row - the sample, the
        bicubic baseline, the corrected sample - over the valid pixels of the truth alone (`metrics.image_quality(nodata=)`)
        and adds "valid_fraction".  The model keeps the train / eval mode it came with.
        `lr_consistency` (a consistency.LRConsistency; not with `ensemble` or `known_mask_fn`) samples every batch with that
        request as `self.lr_consistency` - the "model" row - and a second time without it from the same noise (`noise_source`
        asked again, or torch's generators put back where they were), the "model_free" row; "model", "model_free" and "bicubic"
        gain "lr_rmse", `consistency.lr_rmse` of the estimate clamped to [0, 1] against the batch's LR images.  Without it the
        result is what it was, key for key."""
        self._check_evaluate_nodata(nodata, ensemble, known_mask_fn)
        fix = self._evaluate_color_fix(color_fix, color_fix_levels, ensemble, known_mask_fn)
        consistent = self._evaluate_consistency(lr_consistency, ensemble, known_mask_fn)
        sample, members = self._evaluate_samplers(model, "input_channels", sampling_steps, eta, noise_source, known_mask_fn,
                                                  resample, jump, ensemble, member_batch)
        scorers = {"model": sample}
        if consistent is not None:
            scorers.update(consistent(sample))
        if baseline:
            scorers["bicubic"] = lambda lr_img, hr_img: hip_ops.bicubic_upsample(lr_img, self.magnification_factor)
            if consistent is not None:
                scorers["bicubic"] = consistent.scored(scorers["bicubic"])
        if fix is not None:
            kept = {}  # the batch's sample, as `drawn` keeps the members of an ensemble: "model" runs before "model_fixed"

            model_scorer = scorers["model"]  # (`sample`, or its LR-consistent form, which returns scores of its own as well)

            def sample_kept(lr_img, hr_img):
                out = model_scorer(lr_img, hr_img)
                kept["x"] = out[0] if isinstance(out, tuple) else out
                return out
            scorers["model"] = sample_kept
            scorers["model_fixed"] = lambda lr_img, hr_img: fix(kept["x"], lr_img)
        return self._evaluate(model, loader, n_images, scorers, self.magnification_factor, members, nodata)

    def _evaluate_consistency(self, request, ensemble, known_mask_fn):
        """`evaluate`'s LR-consistent scorers, None without a request: f(sample) -> {"model": the chain with `request` as
        `self.lr_consistency`, "model_free": the plain chain of the same noise}, and `.scored(scorer)`, the scorer with "lr_rmse"
        added; ValueError for a request `evaluate` does not take (checked before anything is sampled)."""
        from .consistency import check_lr_consistency, lr_rmse
        if check_lr_consistency(request) is None:
            return None
        if ensemble is not None or known_mask_fn is not None:
            raise ValueError("evaluate: lr_consistency cannot be combined with ensemble=N or known_mask_fn")
        ops = {}

        def rmse(est, lr_img):
            size = tuple(est.shape[-2:])
            if size not in ops:
                ops[size] = request.operator_for(self, size)
            return {"lr_rmse": lr_rmse(torch.clamp(est, 0, 1), lr_img, ops[size])}
        request.operator_for(self, (self.image_size, self.image_size))  # (ValueError for a degradation without an operator)

        def scored(scorer):
            def with_rmse(lr_img, hr_img):
                est = scorer(lr_img, hr_img)
                return est, rmse(est, lr_img)
            return with_rmse
        cuda = torch.cuda.is_available() and torch.device(self.device).type == "cuda"

        def rng_state():
            return torch.get_rng_state(), (torch.cuda.get_rng_state(self.device) if cuda else None)

        def set_rng_state(state):
            torch.set_rng_state(state[0])
            if cuda:
                torch.cuda.set_rng_state(state[1], self.device)

        def scorers(sample):
            kept = {}

            def with_attribute(value, lr_img, hr_img):
                before, self.lr_consistency = self.lr_consistency, value
                try:
                    return sample(lr_img, hr_img)
                finally:
                    self.lr_consistency = before

            def projected(lr_img, hr_img):
                kept["rng"] = rng_state()
                return with_attribute(request, lr_img, hr_img)

            def free(lr_img, hr_img):
                set_rng_state(kept.pop("rng"))
                return with_attribute(None, lr_img, hr_img)
            return {"model": scored(projected), "model_free": scored(free)}
        scorers.scored = scored
        return scorers

    @staticmethod
    def _check_evaluate_nodata(nodata, ensemble, known_mask_fn):
        if nodata is None:
            return
        hip_ops.nodata_rule(nodata)  # (ValueError for a value that is no rule)
        if ensemble is not None or known_mask_fn is not None:
            raise ValueError("evaluate: nodata cannot be combined with ensemble=N or known_mask_fn: their scores are not masked")

    def _evaluate_color_fix(self, method, levels, ensemble, known_mask_fn):
        """`evaluate`'s f(sample batch, lr batch) -> corrected batch, None without a method; ValueError for a request it does
        not take (checked before anything is sampled)."""
        if method is None:
            return None
        from .colorfix import color_fix, fix_levels
        levels = fix_levels(method, levels)
        if ensemble is not None or known_mask_fn is not None:
            raise ValueError("evaluate: color_fix cannot be combined with ensemble=N or known_mask_fn")
        return lambda x, lr_img: color_fix(torch.clamp(x, 0, 1), lr_img, magnification_factor=self.magnification_factor,
                                           method=method, levels=levels)

    def _evaluate_samplers(self, model, channels_kw, sampling_steps, eta, noise_source, known_mask_fn, resample, jump, ensemble,
                           member_batch):
        """`evaluate`'s (`sample`, `members`), both f(conditioning batch, truth batch): one `sample` / `sample_known` call, and
        one `sample_ensemble` call (None without `ensemble`).  `channels_kw`: the sampler's name for the truth's band count."""
        self._check_evaluate_ensemble(ensemble, member_batch, known_mask_fn)

        def members(cond, truth):
            return self.sample_ensemble(ensemble, model, cond, member_batch=member_batch, sampling_steps=sampling_steps,
                                        eta=eta, noise_source=noise_source, **{channels_kw: truth.shape[1]})

        def sample(cond, truth):
            args = {channels_kw: truth.shape[1], "noise_source": noise_source, "sampling_steps": sampling_steps, "eta": eta}
            if known_mask_fn is None:
                check_inpaint_args(tuple(truth.shape), None, None, resample, jump)
                return self.sample(cond.shape[0], model, cond, **args)
            return self._score_known(truth, known_mask_fn(truth), lambda known, mask: self.sample_known(
                cond.shape[0], model, cond, known, mask, resample=resample, jump=jump, **args))
        return sample, members if ensemble else None

    @staticmethod
    def _check_evaluate_ensemble(ensemble, member_batch, known_mask_fn):
        if ensemble is None:
            if member_batch is not None:
                raise ValueError("member_batch belongs to ensemble=N")
            return
        check_ensemble_args(ensemble, member_batch)
        if ensemble > 32:
            raise ValueError(f"ensemble={ensemble}: the ensemble kernels take at most 32 members")
        if known_mask_fn is not None:
            raise ValueError("evaluate: ensemble=N and known_mask_fn cannot be combined")

    @staticmethod
    def _score_known(truth, mask, sample_known):
        """One batch of `evaluate` with known pixels: `sample_known(known, mask)` with the truth as the known image, and the
        result together with {"psnr_unknown": per-image values over the hidden pixels}."""
        from . import metrics
        mask = mask.to(truth.device)
        out = sample_known(truth, mask)
        return out, {"psnr_unknown": metrics.psnr_masked(out, truth, mask == 0)}

    def _evaluate(self, model, loader, n_images, scorers, magnification_factor, members=None, nodata=None):
        """`evaluate` for the estimators `scorers` = {name: f(conditioning batch, truth batch) -> estimate}.  With `members` =
        f(conditioning batch, truth batch) -> (N, B, C, S, S) the "model" scorer is replaced by the mean of those members,
        "member" scores member 0 and "ensemble" collects `ensemble.ensemble_scores` of the batch."""
        from . import ensemble, metrics
        was_training = model.training
        masked = {} if nodata is None else {"nodata": nodata}  # (None: the call it always was)
        ens = {}
        if members is not None:
            drawn = {}

            def draw(cond, truth):
                drawn["x"] = members(cond, truth)
                ens_b = ensemble.ensemble_scores(drawn["x"], truth, clamp=(0.0, 1.0))
                for k, v in ens_b.items():
                    ens.setdefault(k, []).append(v)
                return hip_ops.ensemble_stats(drawn["x"], None, (0.0, 1.0), std=False)[0]
            scorers = {"model": draw, "member": lambda cond, truth: drawn["x"][0],
                       **{k: f for k, f in scorers.items() if k != "model"}}
        per_image, n = {name: {} for name in scorers}, 0
        for batch in loader:
            cond, truth = self._split_batch(batch)
            if n_images is not None:
                cond, truth = cond[:n_images - n], truth[:n_images - n]
            if truth.shape[0] == 0:
                break
            cond, truth = cond.float().contiguous(), truth.float().contiguous()
            for name, estimate in scorers.items():
                est = estimate(cond, truth)
                est, more = est if isinstance(est, tuple) else (est, {})  # (`_score_known`: scores of its own)
                for k, v in {**metrics.image_quality(est, truth, magnification_factor, **masked), **more}.items():
                    per_image[name].setdefault(k, []).append(v)
            n += truth.shape[0]
            if n_images is not None and n >= n_images:
                break
        model.train(was_training)
        if n == 0:
            raise ValueError("evaluate: the loader holds no image")
        per_image = {name: {k: torch.cat(v) for k, v in d.items()} for name, d in per_image.items()}
        out = {name: {k: v.mean().item() for k, v in d.items()} for name, d in per_image.items()}
        out["per_image"] = {name: {k: v.tolist() for k, v in d.items()} for name, d in per_image.items()}
        if ens:
            ens = {k: torch.cat(v) for k, v in ens.items()}
            out["ensemble"] = {k: (v.sum(dim=0).tolist() if k == "rank_histogram" else v.mean().item()) for k, v in ens.items()}
            out["per_image"]["ensemble"] = {k: v.tolist() for k, v in ens.items()}
        out["n"] = n
        return out

    # -- snapshots (reference :257-308) -----------------------------------------------------------
    def _unwrapped(self, model):
        """The network whose state_dict is saved and loaded: under --multiple_gpus a wrapper's `.module`."""
        return model.module if self.multiple_gpus and hasattr(model, "module") else model

    @staticmethod
    def _engine_net(model):
        """The network that owns the HIP engine: a wrapper's `.module`, unless the wrapper answers `hip_engine` itself."""
        return model.module if hasattr(model, "module") and not hasattr(model, "hip_engine") else model

    def _save_snapshot(self, epoch, model):
        snapshot = {"MODEL_STATE": self._unwrapped(model).state_dict(), "EPOCHS_RUN": epoch}
        if self.prediction != "eps":  # (an eps network's file stays the reference's two keys)
            snapshot["PREDICTION"] = self.prediction
        if self.zero_terminal_snr:  # (likewise: an off run writes what it always wrote)
            snapshot["ZERO_TERMINAL_SNR"] = True
        if getattr(self, "data_range", None) is not None:  # (likewise: only a 16-bit run)
            snapshot["DATA_RANGE"] = self._data_range_key(self.data_range)
        if getattr(self, "mtf_nyquist", None) is not None:  # (likewise: only an MTF run)
            snapshot["MTF_NYQUIST"] = [float(g) for g in self.mtf_nyquist]
        torch.save(snapshot, self.snapshot_path)
        print(f"Epoch {epoch} | Training snapshot saved at {self.snapshot_path}")

    def _load_snapshot(self):
        if self.multiple_gpus:
            from collections import OrderedDict
            snapshot = torch.load(self.snapshot_path, map_location="cpu")
            self._check_snapshot_prediction(snapshot)
            state = OrderedDict((k.replace("module.", ""), v) for k, v in snapshot["MODEL_STATE"].items())
            net = self._unwrapped(self.model)
            net.load_state_dict(state)
            net.to(self.device)
        else:
            snapshot = torch.load(self.snapshot_path, map_location=self.device)
            self._check_snapshot_prediction(snapshot)
            self.model.load_state_dict(snapshot["MODEL_STATE"])
        self.epochs_run = snapshot["EPOCHS_RUN"]
        print(f"Resuming training from snapshot at Epoch {self.epochs_run}")

    def _check_snapshot_prediction(self, snapshot):
        """ValueError for a snapshot of a network that predicts something else than this `Diffusion` was told (a file without
        the key: eps): its weights would be sampled and trained as what they are not."""
        saved = snapshot.get("PREDICTION", "eps")
        if saved != self.prediction:
            raise ValueError(f"{self.snapshot_path} holds a network that predicts {saved!r}, this Diffusion was built with "
                             f"prediction={self.prediction!r} (--prediction {saved})")
        saved = bool(snapshot.get("ZERO_TERMINAL_SNR", False))
        if saved != self.zero_terminal_snr:
            raise ValueError(f"{self.snapshot_path} holds a network trained with zero_terminal_snr={saved}, this Diffusion was "
                             f"built with zero_terminal_snr={self.zero_terminal_snr}: the two schedules differ at every level "
                             f"({'pass' if saved else 'drop'} --zero_terminal_snr)")
        self.snapshot_data_range = snapshot.get("DATA_RANGE")
        self._check_mtf_key(snapshot.get("MTF_NYQUIST"), self.snapshot_path)

    @staticmethod
    def _check_mtf(kind, nyquist, noise, model, magnification_factor):
        """(mtf_nyquist, mtf_noise) of the constructor: (None, None) unless `kind` is "MTF", else per-band tuples, checked
        against the network's band count (a model that does not tell it: the length of the list)."""
        from . import mtf
        if str(kind).lower() != "mtf":
            if nyquist is not None or noise is not None:
                raise ValueError(f"mtf_nyquist / mtf_noise belong to Degradation_type='MTF' (got {kind!r})")
            return None, None
        if nyquist is None:
            raise ValueError("Degradation_type='MTF' needs mtf_nyquist: the gain at the LR Nyquist frequency, one number or one per "
                             "band (--mtf_nyquist)")
        mtf._check_factor(magnification_factor)
        bands = getattr(model, "image_channels", None)
        if bands is None:
            bands = 1 if isinstance(nyquist, (int, float)) else len(nyquist.split(",") if isinstance(nyquist, str) else list(nyquist))
        nyquist = mtf.parse_mtf_nyquist(nyquist, bands)
        return nyquist, (None if noise is None else mtf.parse_mtf_noise(noise, len(nyquist)))

    def _check_mtf_key(self, saved, where):
        """ValueError for a file written under other per-band MTF gains than `self.mtf_nyquist` (None: not an MTF run)."""
        mine = getattr(self, "mtf_nyquist", None)
        saved = None if saved is None else tuple(float(g) for g in saved)
        if saved != (None if mine is None else tuple(float(g) for g in mine)):
            def text(t):
                return "none (not an MTF run)" if t is None else ",".join(f"{g:g}" for g in t)
            raise ValueError(f"{where} was written with --mtf_nyquist {text(saved)}, this run has {text(mine)}: a network goes on "
                             "under the degradation it was trained for")

    @staticmethod
    def _data_range_key(table):
        """A band-range table as the files keep and compare it: None, or a (C, 2) fp32 host tensor."""
        return None if table is None else torch.as_tensor(table, dtype=torch.float32).detach().cpu().reshape(-1, 2).clone()

    def _check_data_range(self, saved, where):
        """ValueError for a run that goes on from a file written under other band ranges than `self.data_range`: its network
        was trained on other numbers for the same pixels."""
        mine = self._data_range_key(getattr(self, "data_range", None))
        if (saved is None) != (mine is None) or (mine is not None and not torch.equal(self._data_range_key(saved), mine)):
            def text(t):
                return "none (an 8-bit run)" if t is None else ";".join(f"{lo:g},{hi:g}" for lo, hi in self._data_range_key(t).tolist())
            raise ValueError(f"{where} was written with --data_range {text(saved)}, this run has {text(mine)}: a resumed run "
                             "must normalise with the same band ranges")

    # -- the rest of a run's state (not in the reference, which marks the gap: LR_SCHEDULER is commented out at :275) --------
    def train_state_path(self):
        return os.path.join(os.path.dirname(self.snapshot_path), "train_state.pt")

    def _save_train_state(self, epoch, run):
        """`train_state.pt` beside the snapshot (whose two keys stay what they are): everything else `train` needs to go on at
        epoch + 1 as if it had not stopped.  With EMA the snapshot holds the averaged copy, so the raw weights are here.  Not
        saved: the private generators of the crop / BSRGAN feeds.  One file, written by rank 0 and read by every rank."""
        ts = {"OPTIMIZER_STATE": run.optimizer.state_dict(),
              "RAW_MODEL_STATE": self._unwrapped(run.model).state_dict() if run.ema is not None else None,
              "EMA_STEP": run.ema.step if run.ema is not None else None,
              "LR_SCHEDULE": run.scheduler.state_dict() if run.scheduler is not None else None,
              "BEST_LOSS": run.best_loss, "EPOCHS_WITHOUT_IMPROVING": run.epochs_without_improving,
              "NEXT_EPOCH": epoch + 1, "CPU_RNG_STATE": torch.get_rng_state(),
              "DEVICE_RNG_STATE": torch.cuda.get_rng_state(self.device)}
        if run.loss_bins is not None:  # (a run without --loss_bins / loss_aware writes the file it always wrote)
            ts["LOSS_BINS"] = run.loss_bins.state_dict()
        if getattr(run, "freeze_bn", False) or getattr(run, "freeze", ()):  # (likewise)
            ts["FREEZE_BN"], ts["FREEZE"] = run.freeze_bn, tuple(run.freeze)
        if self.zero_terminal_snr:  # (likewise)
            ts["ZERO_TERMINAL_SNR"] = True
        if self.nodata is not None:  # (likewise)
            ts["NODATA"] = self._nodata_key(self.nodata)
        if getattr(self, "data_range", None) is not None:  # (likewise)
            ts["DATA_RANGE"] = self._data_range_key(self.data_range)
        if getattr(self, "mtf_nyquist", None) is not None:  # (likewise)
            ts["MTF_NYQUIST"] = [float(g) for g in self.mtf_nyquist]
        torch.save(ts, self.train_state_path())

    def _load_train_state(self, run):
        """Restores `_save_train_state`'s file into a run that `__init__` has already given the snapshot's weights: those stay
        in the EMA copy, the raw weights go into `run.model`, and `epochs_run` becomes NEXT_EPOCH.  A file that does not fit
        this model or this run's options raises ValueError."""
        ts = torch.load(self.train_state_path(), map_location="cpu")
        if (ts["RAW_MODEL_STATE"] is None) != (run.ema is None) or (ts["LR_SCHEDULE"] is None) != (run.scheduler is None):
            raise ValueError(f"{self.train_state_path()} was written with other --ema_smoothing / --lr_schedule options")
        if ("LOSS_BINS" in ts) != (run.loss_bins is not None):
            raise ValueError(f"{self.train_state_path()} was written with other --loss_bins / --timestep_sampling options")
        if (bool(ts.get("FREEZE_BN", False)), tuple(ts.get("FREEZE", ()))) != (getattr(run, "freeze_bn", False),
                                                                                tuple(getattr(run, "freeze", ()))):
            raise ValueError(f"{self.train_state_path()} was written with --freeze_bn {bool(ts.get('FREEZE_BN', False))} "
                             f"--freeze {','.join(ts.get('FREEZE', ())) or '(none)'}: a resumed run must freeze the same")
        if bool(ts.get("ZERO_TERMINAL_SNR", False)) != self.zero_terminal_snr:
            raise ValueError(f"{self.train_state_path()} was written with zero_terminal_snr="
                             f"{bool(ts.get('ZERO_TERMINAL_SNR', False))}: a resumed run must keep the schedule")
        if ts.get("NODATA") != self._nodata_key(self.nodata):
            raise ValueError(f"{self.train_state_path()} was written with nodata={ts.get('NODATA')!r}, this run has "
                             f"nodata={self._nodata_key(self.nodata)!r}: a resumed run must mask the same pixels")
        self._check_data_range(ts.get("DATA_RANGE"), self.train_state_path())
        self._check_mtf_key(ts.get("MTF_NYQUIST"), self.train_state_path())
        if run.loss_bins is not None:
            run.loss_bins.load_state_dict(ts["LOSS_BINS"])  # (other T / bin count: ValueError)
        # (another parameter count or other shapes: ValueError from FusedAdamW.load_state_dict, the first thing loaded)
        run.optimizer.load_state_dict(ts["OPTIMIZER_STATE"])
        if run.ema is not None:
            self._unwrapped(run.model).load_state_dict(ts["RAW_MODEL_STATE"])
            run.ema.step = ts["EMA_STEP"]
        if run.scheduler is not None:
            run.scheduler.load_state_dict(ts["LR_SCHEDULE"])
        run.best_loss, run.epochs_without_improving = ts["BEST_LOSS"], ts["EPOCHS_WITHOUT_IMPROVING"]
        self.epochs_run = ts["NEXT_EPOCH"]
        torch.set_rng_state(ts["CPU_RNG_STATE"])
        torch.cuda.set_rng_state(ts["DEVICE_RNG_STATE"], self.device)
        print(f"Resuming the training state of {self.train_state_path()} at Epoch {self.epochs_run}")

    @staticmethod
    def _nodata_key(nodata):
        """`nodata` as `train_state.pt` keeps and compares it: None, "nan" (the NaN rule alone) or the value as fp32 compares it."""
        if nodata is None:
            return None
        value = hip_ops.nodata_rule(nodata)
        return "nan" if value != value else float(torch.tensor(value, dtype=torch.float32))

    def early_stopping(self, patience, epochs_without_improving):
        if epochs_without_improving >= patience:
            print("Early stopping! Training stopped")
            return True

    # -- training loop (reference :319-511) -------------------------------------------------------
    @staticmethod
    def _loss_function(loss, device=None):
        if loss == "MSE":
            return nn.MSELoss()
        if loss == "MAE":
            return nn.L1Loss()
        if loss == "Huber":
            return nn.HuberLoss()
        if loss == "MSE+Perceptual_noise":
            # 0.3 * MSE + 0.7 * VGG19 perceptual loss of the predicted vs the true noise (:353-356), VGG19 on the HIP path
            from .perceptual import mse_perceptual_noise
            return mse_perceptual_noise(device)
        raise ValueError("The Loss must be either MSE or MAE or Huber or MSE+Perceptual_noise")

    def _objective(self, loss, loss_weighting, min_snr_gamma, timestep_sampling, loss_bins):
        """None for a default run; otherwise what `train` swaps in for the loss module (losses.py): `train` / `val`
        (`DiffusionLoss` with the same table, bins of their own), `bins` / `val_bins` (`LossBins` or None) and `sampler`
        (`LossAwareSampler` or None).  Under --multiple_gpus every rank has its own."""
        if loss_weighting not in ("none", "min_snr") or timestep_sampling not in ("uniform", "loss_aware"):
            raise ValueError("loss_weighting must be none or min_snr, timestep_sampling uniform or loss_aware")
        if loss_bins < 0 or not min_snr_gamma > 0:
            raise ValueError("loss_bins must be >= 0 and min_snr_gamma > 0")
        if loss_weighting == "min_snr" and self.zero_terminal_snr:
            raise ValueError("loss_weighting='min_snr' cannot be combined with zero_terminal_snr: the Min-SNR weight of a v or "
                             "x0 target is 0 at SNR 0, so the terminal level - the one the schedule exists for - would not be "
                             "trained")
        if loss_weighting == "none" and timestep_sampling == "uniform" and not loss_bins:
            return None
        if loss == "MSE+Perceptual_noise":
            raise ValueError("--loss MSE+Perceptual_noise cannot be combined with --loss_weighting / --timestep_sampling / "
                             "--loss_bins: the VGG term has no per-image split")
        if loss not in ("MSE", "MAE", "Huber"):
            raise ValueError("The Loss must be either MSE or MAE or Huber or MSE+Perceptual_noise")
        nbins = loss_bins or (16 if timestep_sampling == "loss_aware" else 0)
        table = (min_snr_weights(self.alpha_hat, min_snr_gamma, self.prediction).to(self.device)
                 if loss_weighting == "min_snr" else None)
        bins = LossBins(self.noise_steps, nbins, self.device) if nbins else None
        val_bins = LossBins(self.noise_steps, nbins, self.device) if nbins else None
        return types.SimpleNamespace(train=DiffusionLoss(loss, table, bins), val=DiffusionLoss(loss, table, val_bins),
                                     bins=bins, val_bins=val_bins,
                                     sampler=LossAwareSampler(bins) if timestep_sampling == "loss_aware" else None)

    @staticmethod
    def _bins_line(stats):
        """The mean loss per timestep bin, lowest-noise bin first, `-` for a bin nothing fell into."""
        line = " ".join("-" if m is None else f"{m:.4g}" for m in stats["mean"])
        return line + (f" | non-finite images {stats['nonfinite']}" if stats["nonfinite"] else "")

    def _is_rank0(self):
        return (not self.multiple_gpus) or self.device == 0 or drs_dist.rank() == 0

    def _predict(self, net, x_t, t, cond):
        """The model call of the loop bodies (:388, :474); the SAR / generation subclasses override it."""
        return net(x_t, t, cond, self.magnification_factor)

    def _split_batch(self, batch):
        """(conditioning, clean image) of one loader item: (lr_img, hr_img) here (:379)."""
        return batch[0].to(self.device), batch[1].to(self.device)

    def train_step(self, model, optimizer, loss_function, lr_img, hr_img, ema=None, ema_model=None, lr_scheduler=None):
        """Loop body of reference :379-396 (called `train_step` in BASELINE.json's north_star).  `lr_scheduler`
        (optim.WarmupCosine; not in the reference) sets this step's learning rate right before the update."""
        lr_img, hr_img = self._split_batch((lr_img, hr_img))
        # same CPU-generator draw as the reference (:384); pinned + non_blocking so that the copy does not make the host
        # wait for the previous step's kernels (a pageable .to(device) is a full synchronisation point)
        sample_w = None
        if self.timestep_sampler is not None:
            # loss-aware draw on the device (losses.LossAwareSampler): consumes the DEVICE generator, not the CPU one
            t, sample_w = self.timestep_sampler.draw(hr_img.shape[0])
        else:
            t = self.sample_timesteps(hr_img.shape[0])
            t = (t.pin_memory() if not t.is_cuda else t).to(self.device, non_blocking=True)
        # (`noise`: the target - eps, v or x0 - of `self.prediction`; `valid`: the mask of a run with `nodata`, else None)
        x_t, noise, valid = self._noised(hr_img, t)
        optimizer.zero_grad()
        predicted_noise = self._predict(model, x_t, t, self._train_cond(lr_img))
        if valid is not None:
            if not isinstance(loss_function, DiffusionLoss):
                raise ValueError("nodata needs a losses.DiffusionLoss as loss_function: torch's modules have no mask")
            train_loss, grad = loss_function.loss_and_grad(predicted_noise, noise, t, sample_w, valid=valid)
            predicted_noise.backward(grad)
        elif isinstance(loss_function, DiffusionLoss):
            # loss and d loss / d prediction from one launch: no second pass for autograd's grad_output
            train_loss, grad = loss_function.loss_and_grad(predicted_noise, noise, t, sample_w)
            predicted_noise.backward(grad)
        else:
            train_loss = loss_function(predicted_noise, noise)
            train_loss.backward()
        if lr_scheduler is not None:
            lr_scheduler.step(optimizer)
        if self.multiple_gpus:
            # ONE in-place all-reduce of the backward's flat gradient buffer on RCCL's stream, overlapped with the
            # optimizer's host-side table build; the update kernel is enqueued behind it
            pending = drs_dist.allreduce_gradients(model, async_op=True)
            if isinstance(optimizer, FusedAdam):
                optimizer.step(grad_ready=pending.wait)
            else:
                pending.wait()
                optimizer.step()
        else:
            optimizer.step()
        if ema is not None:
            ema.step_ema(ema_model, model)
        return train_loss

    def _train_cond(self, cond):
        """Conditioning actually passed to the model in a training / validation step (the generation subclass drops
        the label 10% of the time, like its reference loop)."""
        return cond

    def train(self, lr, epochs, check_preds_epoch, train_loader, val_loader, patience, loss, verbose, eval_metrics=0,
              sampling_steps=None, eta=0.0, weight_decay=0.0, max_grad_norm=None, lr_schedule="constant", warmup_steps=0,
              lr_min=0.0, save_train_state=False, loss_weighting="none", min_snr_gamma=5.0, timestep_sampling="uniform",
              loss_bins=0, freeze_bn=False, freeze=(), init_from=None):
        """`eval_metrics=N` (not in the reference; 0 = off): at every epoch with epoch % check_preds_epoch == 0 the network that
        would be saved is scored on the first N validation images (`evaluate` with `sampling_steps` / `eta`), one line.
        Not in the reference either, all off by default (then this is its loop: Adam at a fixed rate): `weight_decay` and
        `max_grad_norm` (decoupled decay, clipping of the global gradient norm, and a guard that skips a step whose gradients
        are not finite: `optim.FusedAdamW`); `lr_schedule` "constant" | "cosine" with `warmup_steps` and `lr_min`
        (`optim.WarmupCosine` over len(train_loader) * epochs steps); `save_train_state`: every snapshot gets a
        `train_state.pt` beside it and a run that finds both continues exactly where that one stood (`_save_train_state`).
        The objective (losses.py; all off by default, then the loss is torch's module and t the CPU
        generator's uniform draw): `loss_weighting="min_snr"` weights every image's loss with min(1, `min_snr_gamma` / SNR_t);
        `loss_bins=N` keeps the mean loss per timestep bin and prints it, lowest-noise bin first, one more line per phase;
        `timestep_sampling="loss_aware"` draws t on the device from those bins' recent losses (16 bins when `loss_bins` is 0)
        and so consumes the DEVICE generator instead of the CPU one.  Any of them routes `train_step` and the validation loop
        through `losses.DiffusionLoss`; validation keeps its uniform CPU draw of t and has bins of its own.
        The regression target of both loops is what the constructor's `prediction` names (`_noised_target`: eps, v or x0; Min-SNR
        weights that target); `loss="MSE+Perceptual_noise"` needs an eps network (ValueError otherwise).
        Fine-tuning a snapshot (finetune.py; all off by default): `init_from=PATH` starts a run whose own
        snapshot does not exist yet from the MODEL_STATE of that file, at epoch 0; `freeze_bn=True` keeps every BatchNorm2d on
        its running statistics (`model.freeze_batchnorm()`: the frozen train plan, statistics never written);
        `freeze=("downs.", "LR_encoder.")` takes the parameters under those state_dict-key prefixes out of training.
        No-data pixels are not an argument but the attribute `self.nodata` (None: off): with it both loops
        take the mask from `_noised_target` and run `losses.DiffusionLoss(valid=)` - a `DiffusionLoss(loss)` of their own where
        the run would otherwise use torch's module -, `eval_metrics` scores under the truth's mask, `loss="MSE+Perceptual_noise"`
        raises, and `save_train_state` stores the setting."""
        self._check_nodata(loss)  # (before any weight is loaded or frozen)
        if os.path.exists(self.snapshot_path) and (getattr(self, "data_range", None) is not None or
                                                 getattr(self, "snapshot_data_range", None) is not None):
            self._check_data_range(self.snapshot_data_range, self.snapshot_path)  # (a run that goes on from a snapshot)
        self._prepare_finetune(freeze_bn, freeze, init_from)
        run = self._begin_run(
            loss, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, lr_schedule=lr_schedule,
            warmup_steps=warmup_steps, lr_min=lr_min, total_steps=max(len(train_loader), 1) * epochs,
            save_train_state=save_train_state, loss_weighting=loss_weighting, min_snr_gamma=min_snr_gamma,
            timestep_sampling=timestep_sampling, loss_bins=loss_bins, freeze_bn=freeze_bn, freeze=freeze)
        eval_args = {"n_images": eval_metrics, "sampling_steps": sampling_steps, "eta": eta} if eval_metrics else None
        for epoch in range(self.epochs_run, epochs):
            checking = epoch % check_preds_epoch == 0
            train_loss, norm_sum = self._train_epoch(run, epoch, train_loader)
            self._report_train_epoch(run, epoch, train_loss, norm_sum, len(train_loader))
            if val_loader is None:
                if checking and self._is_rank0():
                    self._save(run, epoch)
            else:
                val_loss = self._validation_epoch(run, val_loader)
                self._report_validation(run, epoch, val_loss, val_loader, eval_args if checking else None)
                self._keep_if_best(run, epoch, val_loss)
                if self.early_stopping(patience, run.epochs_without_improving):
                    break
            print("Epochs without improving: ", run.epochs_without_improving)

    def _begin_run(self, loss, *, lr, weight_decay, max_grad_norm, lr_schedule, warmup_steps, lr_min, total_steps,
                   save_train_state, loss_weighting, min_snr_gamma, timestep_sampling, loss_bins, freeze_bn=False, freeze=()):
        """The `TrainRun` of one `train` call, kept as `self.train_state`: optimizer, schedule, EMA copy and objective from its
        arguments (and `self.timestep_sampler`), continued from `train_state.pt` when `save_train_state` finds one."""
        model = self.model
        if lr_schedule not in ("constant", "cosine"):
            raise ValueError("lr_schedule must be constant or cosine")
        if loss == "MSE+Perceptual_noise" and self.prediction != "eps":
            raise ValueError(f"--loss MSE+Perceptual_noise cannot be combined with prediction={self.prediction!r}: its VGG term "
                             "compares the predicted noise with the true noise")
        objective = self._objective(loss, loss_weighting, min_snr_gamma, timestep_sampling, loss_bins)
        if weight_decay or max_grad_norm is not None or save_train_state:
            optimizer = FusedAdamW(model.parameters(), lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        else:
            optimizer = FusedAdam(model.parameters(), lr=lr)  # torch.optim.Adam's math, one launch (optim.py)
        scheduler = None
        if lr_schedule == "cosine" or warmup_steps:
            scheduler = WarmupCosine(lr, warmup_steps, total_steps, lr_min, lr_schedule)
        ema = ema_model = None
        if self.ema_smoothing:
            ema = EMA(beta=0.995)
            ema_model = copy.deepcopy(model).eval().requires_grad_(False)
        if objective is not None:
            loss_function, val_loss_function = objective.train, objective.val
        elif self.nodata is not None:  # the masked launch is DiffusionLoss's: unit weights, no bins
            loss_function, val_loss_function = DiffusionLoss(loss), DiffusionLoss(loss)
        else:
            loss_function, val_loss_function = self._loss_function(loss, self.device), None
        self.timestep_sampler = objective.sampler if objective is not None else None
        run = self.train_state = TrainRun(model, loss, optimizer, scheduler, ema, ema_model, objective, loss_function,
                                          clipping=max_grad_norm is not None, save_train_state=save_train_state)
        run.freeze_bn, run.freeze = bool(freeze_bn), tuple(freeze)
        run.val_loss_function = val_loss_function  # (None: validation calls `loss_function`, torch's module)
        if save_train_state and os.path.exists(self.snapshot_path) and os.path.exists(self.train_state_path()):
            self._load_train_state(run)
        return run

    def _check_nodata(self, loss):
        """ValueError, before any device work of a run, for a `nodata` setting this trainer does not take."""
        if self.nodata is None:
            return
        hip_ops.nodata_rule(self.nodata)
        if loss == "MSE+Perceptual_noise":
            raise ValueError("--loss MSE+Perceptual_noise cannot be combined with nodata: the VGG term has no mask")
        if str(getattr(self, "Degradation_type", "DownBlur")).lower() == "bsrgan":
            raise ValueError("nodata cannot be combined with --Degradation_type BSRGAN: its HR image is sharpened, so a "
                             "no-data value does not survive into the training target")

    def _prepare_finetune(self, freeze_bn, freeze, init_from):
        """What `train`'s `init_from` / `freeze_bn` / `freeze` do to the network before the optimizer and the EMA copy are
        made (finetune.py).  A default call touches nothing and prints nothing."""
        if isinstance(freeze, str):
            raise ValueError("freeze must be a tuple of state_dict-key prefixes, e.g. ('downs.', 'LR_encoder.')")
        freeze = tuple(freeze)
        if not (freeze_bn or freeze or init_from):
            return
        net = self._unwrapped(self.model)
        if init_from and not os.path.exists(self.snapshot_path):  # (the run's own snapshot, loaded by __init__, wins)
            load_init_weights(net, init_from, self.prediction, "cpu" if self.multiple_gpus else self.device)
            net.to(self.device)
            print(f"Starting from the weights of {init_from} at Epoch 0")
        if freeze_bn:
            if not hasattr(net, "freeze_batchnorm"):
                raise ValueError("freeze_bn needs one of the three UNet classes (model.freeze_batchnorm())")
            net.freeze_batchnorm(True)
        (n_off, n_on), (e_off, e_on) = freeze_parameters(net, freeze)
        print(f"Fine-tuning: {n_off} parameter tensors frozen ({e_off} values), {n_on} trained ({e_on} values); BatchNorm "
              f"statistics {'frozen' if freeze_bn else 'updated'}")

    def _save(self, run, epoch):
        self._save_snapshot(epoch, run.saved)
        if run.save_train_state:
            self._save_train_state(epoch, run)

    def _train_epoch(self, run, epoch, train_loader):
        """One pass over `train_loader` through `train_step`: (mean loss, the sum of the pre-clip gradient norms of the steps
        that were not skipped - a device tensor, zero without clipping)."""
        if self.multiple_gpus and hasattr(train_loader, "sampler") and hasattr(train_loader.sampler, "set_epoch"):
            train_loader.sampler.set_epoch(epoch)
        running_train_loss = torch.zeros((), device=self.device)  # accumulated on device: no per-step sync
        running_norm = torch.zeros((), device=self.device)
        run.model.train()
        for lr_img, hr_img in train_loader:
            running_train_loss += self.train_step(run.model, run.optimizer, run.loss_function, lr_img, hr_img, run.ema,
                                                  run.ema_model, run.scheduler).detach()
            if run.clipping:
                running_norm += torch.nan_to_num(run.optimizer.last_grad_norm(), nan=0.0, posinf=0.0, neginf=0.0)
        # (this .item() is the epoch's synchronisation point: a wave of the wave-specialised kernels that gave up on a counter
        #  during this epoch's forwards or backwards - csrc/sp_sync.h - is reported right after it, not trained on)
        return running_train_loss.item() / max(len(train_loader), 1), running_norm

    def _report_train_epoch(self, run, epoch, train_loss, norm_sum, steps):
        """The engine's fault check, then the epoch's train lines: the loss (with the clipping figures), the fused loss's own
        fault check, the loss bins."""
        net = self._engine_net(run.model)
        if hasattr(net, "hip_engine"):
            net.hip_engine().check_faults()
        print(f"Epoch {epoch}: Running Train ({run.loss}) {train_loss}" + self._clipping_report(run, norm_sum, steps))
        if run.objective is not None:
            run.objective.train.check_faults()
        if run.loss_bins is not None:
            print(f"Epoch {epoch}: Train loss by timestep bin (low noise first) "
                  + self._bins_line(run.loss_bins.read_and_reset()))

    @staticmethod
    def _clipping_report(run, norm_sum, steps):
        """` | mean grad norm ... | skipped steps ...` of an epoch of `steps` steps, as far as the run has them."""
        if not isinstance(run.optimizer, FusedAdamW):
            return ""
        skipped = run.optimizer.skipped_steps() - run.skipped_before
        run.skipped_before += skipped
        more = f" | mean grad norm {norm_sum.item() / max(steps - skipped, 1)}" if run.clipping else ""
        return more + (f" | skipped steps {skipped}" if skipped else "")

    def _validation_epoch(self, run, val_loader):
        """The mean loss of the network that would be saved over `val_loader`, with t from the uniform CPU draw; under
        --multiple_gpus the mean over the ranks' means."""
        running_val_loss = torch.zeros((), device=self.device)
        with torch.no_grad():
            run.model.eval()
            for batch in val_loader:
                lr_img, hr_img = self._split_batch(batch)
                t = self.sample_timesteps(hr_img.shape[0]).to(self.device)
                x_t, noise, valid = self._noised(hr_img, t)
                predicted_noise = self._predict(run.saved, x_t, t, self._train_cond(lr_img))
                if valid is not None:
                    running_val_loss += run.val_loss_function(predicted_noise, noise, t, valid=valid)
                elif run.objective is not None:  # the same table through the no-grad path; uniform t, bins of its own
                    running_val_loss += run.objective.val(predicted_noise, noise, t)
                else:
                    running_val_loss += run.loss_function(predicted_noise, noise)
        val_loss = running_val_loss.item() / max(len(val_loader), 1)
        if self.multiple_gpus:
            # the reference decides per rank on its own validation shard (:492-510, quirk Q9); with a collective in
            # every training step the ranks must leave the loop together: one mean over ranks, same branch everywhere
            val_loss = drs_dist.allreduce_mean_scalar(val_loss)
        return val_loss

    def _report_validation(self, run, epoch, val_loss, val_loader, eval_args):
        """The epoch's validation lines: the loss, the loss bins, and - with `eval_args` - the image scores of `run.saved`."""
        print(f"Epoch {epoch}: Running Val loss ({run.loss}){val_loss}")
        if run.loss_bins is not None:
            print(f"Epoch {epoch}: Val loss by timestep bin (low noise first) "
                  + self._bins_line(run.objective.val_bins.read_and_reset()))
        if eval_args is not None:
            scores = self.evaluate(run.saved, val_loader, **eval_args, **({} if self.nodata is None else {"nodata": self.nodata}))
            print(f"Epoch {epoch}: Val metrics on {scores['n']} images | " + format_scores(scores))

    def _keep_if_best(self, run, epoch, val_loss):
        """Early stopping's bookkeeping, the one place that moves it: a new best validation loss is saved (by rank 0)."""
        if val_loss < run.best_loss:
            run.best_loss, run.epochs_without_improving = val_loss, 0
            if self._is_rank0():
                self._save(run, epoch)
        else:
            run.epochs_without_improving += 1


def launch(args):
    """Reference launch (:513-693) for the hot path: model + Diffusion + train + final sampling.  `--dataset_path` is the
    reference's image folder (`<path>/train_original`, `<path>/val_original`, :597-598: decoded once with Pillow into a uint8
    cache on the device, DownBlur / DownBlurNoise per batch on the device) or `synthetic[:N]` / `synthetic_u8[:N]` (seeded
    patches; float pairs / the same device feed)."""
    if args.Degradation_type.lower() not in _DEGRADATIONS:
        raise ValueError("The degradation type must be either BSRGAN or DownBlur or DownBlurNoise or MTF")
    if args.Degradation_type.lower() == "downblur" and args.image_size % args.magnification_factor != 0:
        raise ValueError("The image size must be a multiple of the magnification factor")
    if args.UNet_type.lower() != "residual attention unet":
        raise ValueError("The UNet type must be Residual Attention UNet or Residual MultiHead Attention UNet or "
                         "Residual Visual MultiHeadAttention UNet superres")
    u16 = radiometry.is_u16(radiometry.check_args(args))
    mtf.check_args(args)
    # a 16-bit run: the feed compares the stored integers with --nodata K and marks the target with NaN (the NaN rule alone)
    nodata = (None if getattr(args, "nodata", None) is None else True) if u16 else \
        nodata_u8_value(getattr(args, "nodata", None), args.Degradation_type)
    print("Using multiple GPUs" if args.multiple_gpus else "Using single GPU")
    device = launch_device(args)
    train_loader, val_loader, final_lr = make_superres_feeds(args, device)
    ch = args.inp_out_channels
    r = drs_dist.rank() if args.multiple_gpus else 0

    print("Using Residual Attention UNet")
    model = Residual_Attention_UNet_superres(ch, ch, device).to(device)
    train_kwargs = {}
    if getattr(args, "eval_metrics", 0):
        train_kwargs = {"eval_metrics": args.eval_metrics, "sampling_steps": args.sampling_steps, "eta": args.eta}
    diffusion = train_model(args, Diffusion, model, device, train_loader, val_loader, train_kwargs, nodata=nodata,
                            **({"data_range": train_loader.data_range} if u16 else {}), magnification_factor=args.magnification_factor, Degradation_type=args.Degradation_type,
                            **mtf.diffusion_kwargs(args))
    if r != 0:
        return  # one rank samples and writes models_run/<name>/results/superres_results.pt (every rank holds the same weights)

    def sample(lr_i, **ddim):
        return diffusion.sample(n=1, model=model, lr_img=lr_i, input_channels=ch, generate_video=args.generate_video, **ddim)
    save_final_samples(args, sample, final_lr, "superres_results.pt")


def nodata_u8_value(k, degradation_type):
    """The `nodata` of a super-resolution `Diffusion` for --nodata K (None: None): float32(K) / 255, the bits the uint8 feeds
    give a stored K, so that the rule's fp32 compare finds the HR pixels whose bands all hold K.  DownBlur / DownBlurNoise only:
    ValueError under BSRGAN, whose HR image is sharpened.  The LR image is still made from the stored pixels, K included."""
    if k is None:
        return None
    if not 0 <= int(k) <= 255:
        raise ValueError(f"--nodata {k} must be an integer in 0 .. 255")
    if str(degradation_type).lower() == "bsrgan":
        raise ValueError("--nodata cannot be combined with --Degradation_type BSRGAN: its HR image is sharpened, so the "
                         "no-data value does not survive into the training target")
    return float(torch.tensor(float(int(k)), dtype=torch.float32) / 255)


def build_arg_parser():
    """`base_arg_parser` and the super-resolution flags of the reference (:703-724)."""
    p = base_arg_parser()
    p.add_argument("--inp_out_channels", type=int, default=3)
    p.add_argument("--magnification_factor", type=int)
    p.add_argument("--Degradation_type", type=str, default="DownBlur")
    p.add_argument("--num_crops", type=int, default=1,
                   help="the reference's patches per scene; this trainer's command line (parse_train_args) says what it does here")
    p.add_argument("--Blur_radius", type=str, default="random")
    return p


def parse_train_args(argv=None):
    """The trainer's command line: `build_arg_parser`, the BSRGAN feed's flags, the crop / augmentation flags (`add_augment_args`:
    --num_crops gets its meaning there) and `--eval_metrics`, which one process evaluates (no distributed evaluation: rejected
    together with --multiple_gpus)."""
    p = build_arg_parser()
    add_bsr_args(p)
    add_augment_args(p)
    add_train_args(p)
    add_prediction_args(p, in_help=False)
    add_finetune_args(p)
    add_nodata_args(p, in_help=False, u8=True)
    radiometry.add_radiometry_args(p, in_help=False)
    mtf.add_mtf_args(p, in_help=False)
    next(a for a in p._actions if a.dest == "nodata").type = cli_nodata_u16  # (0 .. 255 without --bit_depth 16: checked below)
    p.add_argument("--eval_metrics", type=int, default=0,
                   help="score the network on the first N validation images (PSNR / SSIM / SAM / ERGAS against the bicubic "
                        "baseline) at every epoch with epoch %% check_preds_epoch == 0; 0 = off")
    args = p.parse_args(argv)
    if args.eval_metrics < 0:
        p.error("--eval_metrics must be >= 0")
    if args.eval_metrics and args.multiple_gpus:
        p.error("--eval_metrics runs in one process: it cannot be combined with --multiple_gpus")
    if args.nodata is not None and args.Degradation_type.lower() == "bsrgan":
        p.error("--nodata cannot be combined with --Degradation_type BSRGAN: its HR image is sharpened")
    check_nodata_depth(p, args)
    try:
        radiometry.check_args(args)
        mtf.check_args(args)
    except ValueError as e:
        p.error(str(e))
    return check_train_args(p, args)


def main(argv=None):
    args = parse_train_args(argv)
    args.snapshot_folder_path = os.path.join(os.curdir, "models_run", args.model_name, "weights")
    launch(args)


if __name__ == "__main__":
    main()
