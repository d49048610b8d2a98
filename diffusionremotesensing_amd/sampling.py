"""The reverse chain all three samplers and the tiler share: its moves (`chain_moves`), the argument checks, the loop with its
fault checks and roll-back (`run_reverse_chain`) and the chain itself (`sample_chain`), whose one `step` takes every move."""
import math
import numbers
import sys
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, hip_ops
from .consistency import chain_projector, check_lr_consistency


def ddim_timesteps(noise_steps, sampling_steps):
    """The S timesteps a DDIM chain visits, descending: [1 + (k * (T - 2)) // (S - 1) for k in range(S)] reversed, or
    [T - 1] for S = 1 (integer arithmetic only).  S = T - 1 visits the ancestral chain's T - 1 .. 1; the step after the
    last entry goes to timestep 0."""
    T, S = int(noise_steps), int(sampling_steps)
    if not 1 <= S <= T - 1:
        raise ValueError(f"sampling_steps={sampling_steps} outside [1, noise_steps - 1 = {T - 1}]")
    if S == 1:
        return [T - 1]
    return [1 + (k * (T - 2)) // (S - 1) for k in reversed(range(S))]


def rescale_zero_terminal_snr(alpha_hat):
    """The alpha_hat table rescaled to zero terminal SNR (Lin et al., "Common Diffusion Noise Schedules and Sample Steps Are
    Flawed", 2024, Algorithm 1), fp32 on the input's device: with s = sqrt(ah) in float64, s' = (s - s[T-1]) s[0] / (s[0] - s[T-1])
    and ah' = s'^2 cast to fp32; ah'[T-1] is exactly 0.0 and ah'[0] is the input's ah[0], bit for bit.  At the last level the
    forward process then returns pure noise, which is what every sampler starts from."""
    ah = torch.as_tensor(alpha_hat)
    if ah.dim() != 1 or ah.numel() < 2:
        raise ValueError("rescale_zero_terminal_snr needs a table of at least 2 levels")
    s = ah.detach().to("cpu", torch.float64).sqrt()
    if not s[0] > s[-1]:
        raise ValueError("rescale_zero_terminal_snr needs alpha_hat[0] > alpha_hat[T - 1]")
    out = (((s - s[-1]) * s[0] / (s[0] - s[-1])) ** 2).to(torch.float32)
    out[-1] = 0.0
    out = out.to(ah.device)
    out[0] = ah[0].to(torch.float32)
    return out


def check_zero_terminal_snr(zero_terminal_snr, prediction):
    """ValueError for a zero-terminal-SNR schedule under an eps network: at alpha_hat == 0 the state is the noise, so the eps
    target is the network's input and its output says nothing about the image."""
    if zero_terminal_snr and prediction == "eps":
        raise ValueError("zero_terminal_snr needs prediction='v' or 'x0': at the terminal level (alpha_hat == 0) the eps target "
                         "is the network's input itself")
    return bool(zero_terminal_snr)


def check_terminal_eta(schedule, eta):
    """ValueError for eta > 1 on a chain that has a terminal level (sqrt((1 - ah_p)(1 - eta^2)) has no real value there)."""
    if getattr(schedule, "zero_terminal_snr", False) and eta > 1:
        raise ValueError(f"eta={eta} > 1 cannot be taken from the terminal level of a zero_terminal_snr schedule: the move's "
                         "variance eta^2 (1 - alpha_hat) would exceed that of the level it reaches")


def check_guidance_rescale(guidance_rescale):
    """ValueError for a `guidance_rescale` outside [0, 1]; the value as a float."""
    if isinstance(guidance_rescale, bool) or not isinstance(guidance_rescale, numbers.Real) or \
            not 0.0 <= float(guidance_rescale) <= 1.0:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} must be a number in [0, 1]")
    return float(guidance_rescale)


PREDICTIONS = ("eps", "v", "x0")


def check_prediction(prediction="eps", x0_clip=None):
    """ValueError for a `prediction` / `x0_clip` no `Diffusion` takes: what the network predicts - "eps", "v" (v = sqrt(ah) eps -
    sqrt(1 - ah) x0) or "x0" - and None or the (lo, hi), lo < hi, the x0 every reverse step implies is clamped to.  Returns
    (prediction, x0_clip as a pair of floats or None)."""
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction={prediction!r} must be one of {PREDICTIONS}")
    if x0_clip is None:
        return prediction, None
    try:
        lo, hi = (float(v) for v in x0_clip)
    except (TypeError, ValueError):
        raise ValueError(f"x0_clip={x0_clip!r} must be None or (lo, hi)") from None
    if not lo < hi:
        raise ValueError(f"x0_clip=({lo}, {hi}) needs lo < hi")
    return prediction, (lo, hi)


def check_threshold(x0_threshold=None, x0_clip=None):
    """ValueError for an `x0_threshold` no `Diffusion` takes: None (off) or the quantile p, 0 < p <= 1, of dynamic thresholding
    (Saharia et al. 2022: per image, the p-quantile s of |x0 - centre of x0_clip|; where s exceeds the half-range the implied x0
    is clamped to centre +- s and rescaled into the range instead of being cut off at it).  A p needs the `x0_clip` that names
    the range.  Returns p as a float, or None."""
    if x0_threshold is None:
        return None
    if isinstance(x0_threshold, bool) or not isinstance(x0_threshold, numbers.Real):
        raise ValueError(f"x0_threshold={x0_threshold!r} must be None or a number in (0, 1]")
    p = float(x0_threshold)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"x0_threshold={x0_threshold!r} must lie in (0, 1]")
    if x0_clip is None:
        raise ValueError(f"x0_threshold={p} needs x0_clip=(lo, hi): the range the image is thresholded to")
    return p


def converts_prediction(predict):
    """Marks a `predict` of `sample_chain` whose result is eps already: it has converted the network's output itself, against
    the x the network saw (the tiler's per-step `predict`, whose network sees tiles and not the chain's scene state)."""
    predict.converts_prediction = True
    return predict


SOLVERS = ("ddim", "dpmpp_2m")
SPACINGS = ("uniform", "logsnr")


class SamplingSteps(int):
    """The `sampling_steps` of a chain that is not plain DDIM: the integer S, which also names the `solver` that takes the S steps
    and the `spacing` of their levels.  It is an int, so everything that hands `sampling_steps` on - `sample_known`,
    `sample_ensemble`, `evaluate`, the tiler, the trainers - hands the solver on with it.  Hand it on as it is: `int(plan)` and
    arithmetic on it (`plan + 1`) give a plain integer, which is DDIM on uniform levels.  ValueError for a name that is no
    solver or spacing, or steps that are no integer.  Usually made by `sampling_plan`."""
    solver = "ddim"
    spacing = None

    def __new__(cls, steps, solver="ddim", spacing=None):
        if solver not in SOLVERS:
            raise ValueError(f"solver={solver!r} must be one of {SOLVERS}")
        if spacing is not None and spacing not in SPACINGS:
            raise ValueError(f"spacing={spacing!r} must be None or one of {SPACINGS}")
        if isinstance(steps, bool) or int(steps) != steps:
            raise ValueError(f"sampling_steps must be an integer, got {steps!r}")
        self = super().__new__(cls, int(steps))
        self.solver, self.spacing = solver, spacing
        return self

    def __repr__(self):
        return f"SamplingSteps({int(self)}, solver={self.solver!r}, spacing={self.spacing!r})"


def sampling_plan(steps, solver="ddim", spacing=None):
    """`sampling_steps=sampling_plan(S, solver="dpmpp_2m")` for `Diffusion.sample` and everything that takes its
    `sampling_steps`: S steps of `solver` - "ddim" or "dpmpp_2m" (DPM-Solver++(2M): second order, one forward per step,
    deterministic) - on levels placed by `spacing`: "uniform" in t (`ddim_timesteps`), "logsnr" (`logsnr_timesteps`) or None,
    which is uniform for "ddim" and logsnr for "dpmpp_2m".  A plain integer S is `sampling_plan(S)`: DDIM on uniform levels.
    ValueError as `SamplingSteps`, and for a solver or spacing without steps."""
    if steps is None:
        raise ValueError(f"solver={solver!r} / spacing={spacing!r} belong to a chain of sampling_steps levels: pass the steps")
    return SamplingSteps(steps, solver, spacing)


def plan_of(sampling_steps):
    """(solver, spacing) of a `sampling_steps` argument, the spacing resolved; ("ddim", "uniform") for a plain integer or None."""
    solver = getattr(sampling_steps, "solver", "ddim")
    spacing = getattr(sampling_steps, "spacing", None)
    return solver, spacing if spacing is not None else ("logsnr" if solver == "dpmpp_2m" else "uniform")


def host_alpha_hat(schedule):
    """The float64 host copy of `schedule.alpha_hat`, kept on the schedule object next to the table it was read from and
    read back again only when another tensor stands there: one read-back per schedule, not one per chain (a read-back makes
    the host wait for everything enqueued on the current stream).  A schedule's table is replaced, never edited in place."""
    ah = schedule.alpha_hat
    held = getattr(schedule, "_alpha_hat_host", None)
    if held is None or held[0] is not ah:
        held = schedule._alpha_hat_host = (ah, torch.as_tensor(ah).detach().to("cpu", torch.float64))
    return held[1]


def logsnr_timesteps(alpha_hat, sampling_steps):
    """S levels, descending and distinct, in [1, T - 1], as uniform in lam_t = 0.5 ln(ah_t / (1 - ah_t)) as the table allows
    (float64 arithmetic on the fp32 table; a device table is read back, so callers with a chain to run hand in a host copy): for each of linspace(lam_{T-1}, lam_1, S) the nearest t
    (ties: the larger t), then t_k = min(t_k, t_{k-1} - 1) going down the list and t_k = max(t_k, S - k) going back up, so
    that the last entry is at least 1.  The step after the last entry goes to level 0, as after `ddim_timesteps`.
    On a zero-terminal-SNR table (ah_{T-1} == 0: lam_{T-1} = -inf, which never enters the linspace) the list is T - 1 followed by
    the S - 1 levels this rule gives on the table restricted to the levels 0 .. T - 2."""
    ah = torch.as_tensor(alpha_hat).detach().to("cpu", torch.float64)
    T, S = ah.numel(), int(sampling_steps)
    if not 1 <= S <= T - 1:
        raise ValueError(f"sampling_steps={sampling_steps} outside [1, noise_steps - 1 = {T - 1}]")
    if float(ah[-1]) == 0.0:
        return [T - 1] + (logsnr_timesteps(ah[:-1], S - 1) if S > 1 else [])
    ah = ah.numpy()
    lam = 0.5 * np.log(ah[1:] / (1.0 - ah[1:]))  # lam[t - 1] = lam_t, decreasing in t
    targets = np.linspace(lam[-1], lam[0], S)
    dist = np.abs(lam[None, ::-1] - targets[:, None])  # (S, T - 1), column j: t = T - 1 - j
    ts = [T - 1 - int(j) for j in np.argmin(dist, axis=1)]  # the nearest t; np.argmin takes the first: the larger t of a tie
    for k in range(1, S):
        ts[k] = min(ts[k], ts[k - 1] - 1)
    for k in range(S - 1, -1, -1):
        ts[k] = max(ts[k], S - k)
    return ts


def chain_levels(noise_steps, sampling_steps=None, spacing="uniform", alpha_hat=None):
    """The levels a chain visits, descending, without the final 0: the ancestral T - 1 .. 1 (`sampling_steps` None), the
    `ddim_timesteps`, or the `logsnr_timesteps` of `alpha_hat`."""
    if sampling_steps is None:
        return list(range(int(noise_steps) - 1, 0, -1))
    if spacing == "logsnr":
        if alpha_hat is None or len(alpha_hat) != noise_steps:
            raise ValueError("spacing='logsnr' needs the alpha_hat table of the noise_steps levels")
        return logsnr_timesteps(alpha_hat, sampling_steps)
    return ddim_timesteps(noise_steps, sampling_steps)


def check_sampling_args(noise_steps, sampling_steps, eta):
    """ValueError for a DDIM or DPM-Solver++(2M) request `Diffusion.sample` cannot run (checked before the engine is touched)."""
    if sampling_steps is not None:
        if isinstance(sampling_steps, bool) or int(sampling_steps) != sampling_steps:
            raise ValueError(f"sampling_steps must be an integer, got {sampling_steps!r}")
        if not 1 <= sampling_steps <= noise_steps - 1:
            raise ValueError(f"sampling_steps={sampling_steps} outside [1, noise_steps - 1 = {noise_steps - 1}]")
    if not (math.isfinite(eta) and eta >= 0):
        raise ValueError(f"eta={eta} must be finite and >= 0")
    if plan_of(sampling_steps)[0] == "dpmpp_2m" and eta > 0:
        raise ValueError(f"solver='dpmpp_2m' is deterministic: eta={eta} must be 0")


def check_solver_known(sampling_steps, known, known_mask):
    """ValueError for known pixels on a DPM-Solver++(2M) chain (checked before the engine is touched)."""
    if plan_of(sampling_steps)[0] == "dpmpp_2m" and (known is not None or known_mask is not None):
        raise ValueError("solver='dpmpp_2m' cannot keep known pixels: their replacement and the forward jumps of the "
                         "resampling invalidate the multistep history (use solver='ddim' or the ancestral chain)")


def check_chain_consistency(schedule, update=None, lr_img=None, needs_lr=False):
    """The `lr_consistency` of `schedule` (None when it has none) for `sample_chain`; ValueError for a value that is no
    `consistency.LRConsistency`, for the per-step `update` hook of the tiler (its state is a scene, its LR images are tiles) and -
    `needs_lr` - for a chain without an LR image: only the super-resolution sampler has an observation to be consistent with; and
    for a degradation the request has no operator for (`LRConsistency.check_for`)."""
    request = check_lr_consistency(getattr(schedule, "lr_consistency", None))
    if request is None:
        return None
    if update is not None:
        raise ValueError("lr_consistency cannot be combined with a per-step update hook (the tiler's aggregation='per_step'): "
                         "the hook blends tiles into a scene state, and no tile's LR image describes it; use aggregation='final', "
                         "or the tiler's own lr_consistency= for the finished scene")
    if needs_lr and lr_img is None:
        raise ValueError("lr_consistency belongs to the super-resolution sampler: this chain has no LR image to be consistent with")
    request.check_for(schedule)
    return request


def check_terminal_chain(schedule, prediction, eta, update=None):
    """(the terminal level of `schedule` or None, its guidance_rescale) for `sample_chain`; ValueError for a chain on a
    zero-terminal-SNR schedule that cannot run: an eps network, eta > 1, or the per-step `update` hook of the tiler, whose
    per-tile conversion to eps is 0 / 0 at the terminal level."""
    phi = check_guidance_rescale(getattr(schedule, "guidance_rescale", 0.0))
    if not getattr(schedule, "zero_terminal_snr", False):
        return None, phi
    check_zero_terminal_snr(True, prediction)
    check_terminal_eta(schedule, eta)
    if update is not None:
        raise ValueError("zero_terminal_snr cannot be combined with a per-step update hook (the tiler's "
                         "aggregation='per_step'): its per-tile conversion to eps is 0 / 0 at the terminal level; use "
                         "aggregation='final'")
    return int(schedule.noise_steps) - 1, phi


def ddim_chain_noise(eta, t, t_prev, shape, x, noise_source):
    """Noise of the DDIM move t -> t_prev: drawn only when sigma > 0 (eta > 0 and t_prev > 0), from `noise_source(t, shape)`
    or torch.randn_like(x); None otherwise, so an eta = 0 chain draws x_T and nothing else."""
    if eta > 0 and t_prev > 0:
        return noise_source(t, shape).to(x.device) if noise_source is not None else torch.randn_like(x)
    return None


def inpaint_schedule(S, resample=1, jump=1):
    """The moves of a chain with known pixels (RePaint, Lugmayr et al., CVPR 2022, Algorithm 1) over the positions 0 .. S of
    its level list (position p holds level L[p]: the ancestral T - 1 .. 1 or the `ddim_timesteps`, then 0): a list of
    (p, q) pairs, q = p + 1 for a reverse move and q = p - jump for a forward jump.  The walk goes down from 0 to S; on its
    FIRST arrival at a position p with p % jump == 0 and 0 < p < S it goes, `resample - 1` times, one jump up to p - jump
    and `jump` moves down again.  That is S + (resample - 1) * jump * ((S - 1) // jump) moves down and (resample - 1) *
    ((S - 1) // jump) up, none of them up from level 0; resample = 1 is the plain replacement chain whatever `jump` is."""
    moves, seen, p = [], set(), 0
    while p < S:
        moves.append((p, p + 1))
        p += 1
        if 0 < p < S and p % jump == 0 and p not in seen:
            seen.add(p)
            for _ in range(resample - 1):
                moves.append((p, p - jump))
                moves.extend((q, q + 1) for q in range(p - jump, p))
    return moves


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and int(v) == v


def check_inpaint_args(shape, known, known_mask, resample=1, jump=1):
    """ValueError for a known-pixel request `Diffusion.sample` cannot run on chains of `shape` = (n, C, S, S) (checked before
    the engine is touched): `known` without `known_mask` or the reverse, a `known` that does not broadcast to (n, C, S, S) or
    a mask that does not to (n, 1 | C, S, S), `resample` / `jump` that are no integers >= 1, or that are set without `known`."""
    for name, v in (("resample", resample), ("jump", jump)):
        if not _is_int(v) or v < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    if (known is None) != (known_mask is None):
        raise ValueError("known and known_mask go together: got " + ("known without known_mask" if known_mask is None
                                                                      else "known_mask without known"))
    if known is None:
        if resample != 1 or jump != 1:
            raise ValueError(f"resample={resample} / jump={jump} belong to a chain with known pixels: pass known and known_mask")
        return
    n, C, H, W = shape
    ks, ms = tuple(known.shape), tuple(known_mask.shape)
    if ks not in ((C, H, W), (n, C, H, W)):
        raise ValueError(f"known {ks} does not broadcast to {(n, C, H, W)}: pass (C, S, S) or (n, C, S, S)")
    if ms not in ((H, W), (1, H, W), (C, H, W), (n, 1, H, W), (n, C, H, W)):
        raise ValueError(f"known_mask {ms} does not broadcast to {(n, 1, H, W)} or {(n, C, H, W)}")


def known_tensors(shape, known, known_mask, device):
    """(`known` as (n, C, S, S) fp32, `known_mask` as (n, 1 | C, S, S) uint8 with 1 = known) on the device, for the update
    kernel: bool, uint8 or {0, 1} float masks, broadcast over the n chains, converted once per chain."""
    n, C, H, W = shape
    known = known.to(device=device, dtype=torch.float32).expand(n, C, H, W).contiguous()
    m = known_mask.to(device)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() == 3:
        m = m.unsqueeze(0)
    return known, (m != 0).to(torch.uint8).expand(n, m.shape[1], H, W).contiguous()


def check_ensemble_args(n_members, member_batch):
    """ValueError for an ensemble request `Diffusion.sample_ensemble` cannot run (checked before the engine is touched)."""
    if not _is_int(n_members) or n_members < 2:
        raise ValueError(f"n_members must be an integer >= 2, got {n_members!r} (`sample` draws a single sample)")
    if member_batch is not None and (not _is_int(member_batch) or member_batch < 1):
        raise ValueError(f"member_batch must be an integer >= 1, got {member_batch!r}")


def ensemble_chunks(n_members, member_batch=None):
    """The members per `sample` call of `Diffusion.sample_ensemble`: `member_batch` at a time (None: all at once), the rest in
    the last call - [2, 2, 1] for 5 members in chunks of 2."""
    m = int(n_members if member_batch is None else min(member_batch, n_members))
    return [min(m, int(n_members) - k) for k in range(0, int(n_members), m)]


def _repeat_members(t, m):
    """A per-chain (B, ...) 4-D tensor repeated for m members, member-major; anything that broadcasts over the chains as is."""
    return t.repeat(m, 1, 1, 1) if t is not None and t.dim() == 4 else t


CHAIN_CHECK_EVERY = 128  # reverse steps between two reads of the kernels' fault word inside a sampling chain


def run_reverse_chain(engine, x, noise_steps, step, frames=None, every=CHAIN_CHECK_EVERY, timesteps=None):
    """The reverse loop of `Diffusion.sample` (reference :234-251): `step(i)` performs reverse step i in place on x, for i =
    noise_steps - 1 .. 1, or for every entry of the list `timesteps` (the descending timesteps of a DDIM chain, or the moves of
    a chain with known pixels: `inpaint_schedule`).  Every `every` steps (and at
    the end) the fault word of the wave-specialised kernels is read (one 4-byte copy + a stream synchronisation: ~0.1 ms per
    128 steps of ~1.2 ms each).  A protocol fault raises.  DRS_ERR_RANGE - an activation left the range of the FL arithmetic's
    fp16 main operand (csrc/conv_mfma_fl.hip; chains of UNTRAINED weights do that, their amplitude grows without bound) - has
    already switched the plan to the split-bf16 kernels: the chain goes back to its last checkpoint (x as of the last clean
    check, a position in the step list) and continues from there."""
    seq = range(noise_steps - 1, 0, -1) if timesteps is None else list(timesteps)
    k = 0
    ckpt_k, ckpt_x, ckpt_frames, since = k, x.clone(), 0, 0
    while k < len(seq):
        step(seq[k])
        k += 1
        since += 1
        if since >= every or k == len(seq):
            since = 0
            try:
                engine.check_faults()
            except _lib.RangeFault as e:
                print(f"[drs] {e}\n[drs] resuming the chain at step {seq[ckpt_k]} on the split-bf16 kernels", file=sys.stderr)
                x.copy_(ckpt_x)
                k = ckpt_k
                if frames is not None:
                    del frames[ckpt_frames:]
                continue
            ckpt_k = k
            ckpt_x.copy_(x)
            ckpt_frames = len(frames) if frames is not None else 0
    return x


def asks_for_known_pixels(known, known_mask, resample, jump, required=False):
    """Whether a request names anything of a chain with known pixels; ValueError if it must (`sample_known`) and does not."""
    asks = not (known is None and known_mask is None and resample == 1 and jump == 1)
    if required and not asks:
        raise ValueError("sample_known needs known and known_mask (`sample` draws a whole image)")
    return asks


class Move(NamedTuple):
    """A reverse step (t_to < t) or a forward jump (t_to > t) of a chain; `run_reverse_chain`'s roll-back line prints its t."""
    t: int
    t_to: int

    def __str__(self):
        return str(self.t)


def chain_moves(noise_steps, sampling_steps=None, resample=1, jump=1, spacing="uniform", alpha_hat=None):
    """The moves of a chain, in order, over its levels: the ancestral T - 1 .. 1 (`sampling_steps` None), the `ddim_timesteps`
    or - `spacing` "logsnr" - the `logsnr_timesteps` of `alpha_hat`, then 0 (`chain_levels`).  Without resampling it steps from
    each level to the next; `resample` / `jump` walk them as `inpaint_schedule` says."""
    levels = chain_levels(noise_steps, sampling_steps, spacing, alpha_hat) + [0]
    return [Move(levels[p], levels[q]) for p, q in inpaint_schedule(len(levels) - 1, resample, jump)]


def sample_chain(schedule, engine, shape, predict, *, table_rows, noise_source=None, sampling_steps=None, eta=0.0,
                 cfg_scale=0.0, update=None, known=None, known_mask=None, resample=1, jump=1, frames=None, lr_img=None):
    """The reverse chain from x_T to the returned x_0 (arguments: `Diffusion._sample_chain`).  `schedule` holds noise_steps, the
    alpha / alpha_hat / beta tables and their device (a Diffusion); `frames`, when a list, gets a copy of x after every move.
    One `step` takes every move of `chain_moves`.  A forward jump to level t_to is one `renoise_` with the draw for t_to.  A
    reverse move t -> t_to is one `predict`, at most one draw - for t - and the `update` hook or one `hip_ops.reverse_step_`;
    it draws iff it ends above level 0 and adds noise there: always on the ancestral chain and with known pixels (whose
    forward noise it also is), on a DDIM chain without them only when eta > 0.  With known pixels the `update` hook also gets
    `known=` / `known_mask=`, converted by `known_tensors` for the chain's `shape` (the tiler's scene), and the move's draw.
    `sampling_steps` may be a `sampling_plan`; its solver "dpmpp_2m" (DPM-Solver++(2M): eta = 0, no known pixels: checked
    by the caller, `check_sampling_args` in every `Diffusion._sample` and `check_solver_known` in `_sample_chain`) takes every
    move with `hip_ops.dpm_step_` - or the `update` hook, which then also gets `hist=` and `t_q=` - and draws nothing but x_T.
    The chain owns the history `hist` (state shape, allocated once: the x0 prediction of the move that wrote it last) and
    `hist_level`, that move's t.  A move is second order iff `hist_level` is the level before its t in the level list and it does
    not end at level 0; so the first move is first order, and so is the move a roll-back of `run_reverse_chain` resumes at
    (the history then holds the x0 of a later move).  Its spacing places the levels (`plan_of`).
    `schedule.prediction` ("eps" when it has none) says what `predict` returns and `schedule.x0_clip` (None or (lo, hi)) what the
    x0 it implies is clamped to.  With anything but "eps" / None the result of `predict` is turned into eps right after the
    call, in place, against the x it was called with (one `hip_ops.pred_to_eps_`, which also forms the guided prediction: the
    update then gets one eps and cfg_scale 0), so every move above takes what it always took; a `predict` marked by
    `converts_prediction` has done so itself.  With "eps" and None nothing is launched.  `schedule.x0_threshold` (None when
    it has none; a quantile p needs the clip: `check_threshold`) makes that one call threshold the implied x0 per image instead
    of clamping it (`pred_to_eps_(..., x0_threshold=p)`); nothing else in the chain changes.
    `schedule.zero_terminal_snr` (False when it has none; read from the schedule, not from the device table: no synchronisation)
    makes level noise_steps - 1 the terminal one, where alpha_hat is 0: a reverse move away from it - the first of every chain,
    and the one after a forward jump back up to it - skips `pred_to_eps_` and the update and is one `hip_ops.terminal_step_`
    on the raw prediction (with the clip, the per-image `hip_ops.x0_abs_quantile` scales under `x0_threshold`, the move's draw,
    the known pixels and, under "dpmpp_2m", the history, after which `hist_level` is None: the next move is first order).  On
    the ancestral chain that move is taken as eta = 1, the true posterior at beta = 1.  The `update` hook cannot take it
    (ValueError: `check_terminal_chain`).  `schedule.guidance_rescale` = phi in (0, 1] (0 when it has none) acts where `predict`
    returns a pair and cfg_scale > 0: one `hip_ops.cfg_rescale` forms the rescaled guided prediction first, and everything after
    it sees a single prediction and cfg_scale 0.
    `schedule.lr_consistency` (None when it has none; a `consistency.LRConsistency`, super-resolution only: it needs `lr_img`, the
    (n | 1, C, h, w) observation of the chains) makes every reverse move below the terminal level LR-consistent: the conversion
    above always runs, and right after it - before the move's draw and the update - one `hip_ops.lr_consistent_eps_` replaces eps
    by that of the implied x0 projected onto the images the degradation maps to `lr_img`.  The projector
    is cached per image size, magnification, radius, damping and device (`consistency.chain_projector`), the observation is
    taken into its basis once per chain.  The terminal move is left as it is: its x0-form step has no eps to correct, and the
    moves after it pull the sample onto the observation.  The `update` hook cannot be combined with it (ValueError)."""
    ddim = sampling_steps is not None
    solver, spacing = plan_of(sampling_steps)
    dpm = solver == "dpmpp_2m"
    prediction, x0_clip = check_prediction(getattr(schedule, "prediction", "eps"), getattr(schedule, "x0_clip", None))
    x0_threshold = check_threshold(getattr(schedule, "x0_threshold", None), x0_clip)
    dynamic = {"x0_threshold": x0_threshold} if x0_threshold is not None else {}
    convert = (prediction != "eps" or x0_clip is not None) and not getattr(predict, "converts_prediction", False)
    terminal_level, phi = check_terminal_chain(schedule, prediction, eta, update)
    consistency = check_chain_consistency(schedule, update, lr_img, needs_lr=True)
    convert = convert or (consistency is not None and not getattr(predict, "converts_prediction", False))
    moves = chain_moves(schedule.noise_steps, sampling_steps, resample, jump, spacing, host_alpha_hat(schedule) if ddim else None)
    with torch.no_grad():
        x = noise_source(schedule.noise_steps, shape) if noise_source is not None else torch.randn(shape)  # (CPU generator, :230)
        x = x.to(schedule.device).contiguous()
        t_rows = hip_ops.timestep_table(schedule.noise_steps, table_rows, x.device)
        if known is not None:
            known, known_mask = known_tensors(shape, known, known_mask, x.device)
        state = {"first": True, "hist_level": None}  # (`first` is not set again after a roll-back)
        hist = torch.empty_like(x) if dpm else None
        level_before = {m.t: before.t for before, m in zip(moves, moves[1:])} if dpm else {}
        projector = yt = None
        if consistency is not None:
            projector = chain_projector(schedule, consistency, shape[2:], x.device)
            lr = lr_img.to(device=x.device, dtype=torch.float32)
            yt = projector.prepare((lr if lr.dim() == 4 else lr.unsqueeze(0)).expand(shape[0], -1, -1, -1).contiguous())

        def draw(t):
            return noise_source(t, shape).to(x.device) if noise_source is not None else torch.randn_like(x)

        def step(move):
            t, t_to = move
            if t_to > t:
                hip_ops.renoise_(x, draw(t_to), t, t_to, schedule.alpha_hat)
            else:
                eps = predict(engine, x, t_rows[t], state["first"])
                state["first"] = False
                eps, eps_uncond = eps if isinstance(eps, tuple) else (eps, None)
                guide = cfg_scale
                if phi > 0 and eps_uncond is not None and cfg_scale > 0:  # (one prediction from here on, as after `convert`)
                    eps = hip_ops.cfg_rescale(eps, eps_uncond, cfg_scale, phi, out=eps)
                    eps_uncond, guide = None, 0.0
                if t == terminal_level:
                    noise = draw(t) if t_to > 0 and (known is not None or not ddim or eta > 0) else None
                    scale = None
                    if x0_threshold is not None:
                        scale = hip_ops.x0_abs_quantile(eps, x, t_rows[t][:shape[0]], schedule.alpha_hat, prediction, x0_clip,
                                                        x0_threshold, pred_uncond=eps_uncond, cfg_scale=guide)
                    hip_ops.terminal_step_(x, eps, noise, t, t_to, schedule.alpha_hat, prediction, eta=eta if ddim else 1.0,
                                           x0_clip=x0_clip, scale=scale, pred_uncond=eps_uncond, cfg_scale=guide, known=known,
                                           known_mask=known_mask, hist=hist)
                    state["hist_level"] = None  # (the next DPM-Solver++(2M) move is first order)
                    if frames is not None:
                        frames.append(x.clone())
                    return
                if convert:  # (the generation sampler's rows are 2n wide: conditional | unconditional)
                    eps = hip_ops.pred_to_eps_(eps, x, t_rows[t][:shape[0]], schedule.alpha_hat, prediction, x0_clip,
                                               pred_uncond=eps_uncond, cfg_scale=cfg_scale, **dynamic)
                    eps_uncond, guide = None, 0.0
                if projector is not None:
                    hip_ops.lr_consistent_eps_(eps, x, t_rows[t][:shape[0]], schedule.alpha_hat, yt, projector, consistency.strength)
                noise = draw(t) if t_to > 0 and (known is not None or not ddim or eta > 0) else None
                if dpm:
                    second = t_to > 0 and state["hist_level"] is not None and state["hist_level"] == level_before.get(t)
                    order = {"hist": hist, "t_q": state["hist_level"] if second else -1}
                    state["hist_level"] = t
                    if update is not None:
                        update(x, eps, None, t, t_to, **order)
                    else:
                        hip_ops.reverse_step_(x, eps, None, t, t_to, alpha=schedule.alpha, alpha_hat=schedule.alpha_hat,
                                              beta=schedule.beta, ddim=True, eps_uncond=eps_uncond, cfg_scale=guide, **order)
                elif update is not None:
                    kept = {"known": known, "known_mask": known_mask} if known is not None else {}
                    update(x, eps, noise, t, t_to if ddim else None, **kept)
                else:
                    hip_ops.reverse_step_(x, eps, noise, t, t_to, alpha=schedule.alpha, alpha_hat=schedule.alpha_hat,
                                          beta=schedule.beta, ddim=ddim, eta=eta, eps_uncond=eps_uncond, cfg_scale=guide,
                                          known=known, known_mask=known_mask)
            if frames is not None:
                frames.append(x.clone())
        run_reverse_chain(engine, x, schedule.noise_steps, step, frames, timesteps=moves)
    return x
