"""The training objective on the device (not in the reference, which trains on a plain `nn.MSELoss`
over uniformly drawn timesteps): Min-SNR-gamma weighting of the per-image loss (`min_snr_weights`; Hang et al. 2023), a
per-timestep-bin loss table (`LossBins`) and the loss-aware timestep draw that reads it (`LossAwareSampler`; the
loss-second-moment resampler of Nichol & Dhariwal 2021, per bin).  `DiffusionLoss` is the launch behind them
(`drs_diffusion_loss`): loss value, gradient and per-image losses from one pass over (pred, target), no host synchronisation.
All of it is off in a default training run.  Tensors must live on a ROCm device: there is no eager fallback.
"""
import ctypes as C

import torch

from . import _lib

KINDS = {"MSE": 0, "MAE": 1, "Huber": 2}  # include/drs_hip.h: DRS_LOSS_*
CHUNK = 4096  # elements per block of the streaming pass (csrc/loss.hip): one partial per chunk and image
MAX_BINS, MAX_HISTORY = 64, 32


def snr(alpha_hat):
    """Signal-to-noise ratio alpha_hat / (1 - alpha_hat) per timestep, (T,) fp32 computed in float64; +inf where
    alpha_hat == 1 (t = 0 of the cosine schedule)."""
    a = alpha_hat.detach().to("cpu", torch.float64)
    return (a / (1.0 - a)).to(torch.float32)


def min_snr_weights(alpha_hat, gamma=5.0, prediction="eps"):
    """Min-SNR-gamma weights of the loss on what the network predicts, (T,) fp32 computed in float64: min(SNR_t, gamma) over
    SNR_t for "eps" (= min(1, gamma / SNR_t)), over SNR_t + 1 for "v", over 1 for "x0" - one weighting of the x0 error, stated
    for each target (Hang et al. 2023, section 3.4).  Where alpha_hat == 1 (SNR = inf) they are 0, 0 and gamma, never NaN."""
    a = alpha_hat.detach().to("cpu", torch.float64)
    if prediction == "eps":
        return torch.clamp(float(gamma) / (a / (1.0 - a)), max=1.0).to(torch.float32)
    if prediction not in ("v", "x0"):
        raise ValueError(f"prediction={prediction!r} must be one of ('eps', 'v', 'x0')")
    capped = torch.clamp(a / (1.0 - a), max=float(gamma))
    # v: min(SNR, gamma) / (SNR + 1), and SNR + 1 = 1 / (1 - alpha_hat): no inf / inf where alpha_hat == 1
    return (capped * (1.0 - a) if prediction == "v" else capped).to(torch.float32)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _masked(valid):
    """The keyword of `DiffusionLoss._launch` for a mask; none without one, so that an unmasked call reaches `_launch` with
    the five positional arguments it always had - code that wraps or replaces `_launch` with that signature keeps working."""
    return {} if valid is None else {"valid": valid}


class LossBins:
    """Per-timestep-bin statistics of the unweighted per-image losses, bin(t) = t * nbins // T, kept on the device and updated by
    the loss launch itself: per bin a double sum and a count (`read_and_reset`), and a ring of the last `history` losses (what
    `LossAwareSampler` draws from).  One 8-byte-word buffer, laid out as include/drs_hip.h says."""

    def __init__(self, T, nbins, device, history=10):
        T, nbins, history = int(T), int(nbins), int(history)
        if not (2 <= nbins <= MAX_BINS and nbins <= T // 2):
            raise ValueError(f"LossBins: need 2 <= nbins <= {MAX_BINS} and nbins <= T // 2, got nbins={nbins} T={T}")
        if not 1 <= history <= MAX_HISTORY:
            raise ValueError(f"LossBins: history={history} outside 1 .. {MAX_HISTORY}")
        if torch.device(device).type != "cuda":
            raise RuntimeError("LossBins: the bins live on a ROCm device (there is no CPU path)")
        self.T, self.nbins, self.history = T, nbins, history
        self.buf = torch.zeros(3 * nbins + 1 + nbins * history, dtype=torch.float64, device=device)

    def _words(self, host):
        n = self.nbins
        as_int = host.view(torch.int64)
        return host[:n], as_int[n:2 * n], as_int[2 * n:3 * n], int(as_int[3 * n]), host[3 * n + 1:].view(n, self.history)

    def read_and_reset(self):
        """{"mean": per-bin mean loss (None for an empty bin), "count": per-bin counts, "nonfinite": images whose loss was not
        finite} since the last call; the ring stays.  Synchronises: for the end of an epoch."""
        total, count, _, nonfinite, _ = self._words(self.buf.cpu())
        n = self.nbins
        self.buf[:2 * n].zero_()
        self.buf[3 * n].zero_()
        count = count.tolist()
        return {"mean": [s / c if c else None for s, c in zip(total.tolist(), count)], "count": count, "nonfinite": nonfinite}

    def ring(self):
        """Per bin the losses its ring holds, oldest first (at most `history`).  Synchronises."""
        _, _, appended, _, ring = self._words(self.buf.cpu())
        out = []
        for k, a in enumerate(appended.tolist()):
            row = ring[k].tolist()
            out.append(row[:a] if a < self.history else row[a % self.history:] + row[:a % self.history])
        return out

    def state_dict(self):
        return {"T": self.T, "nbins": self.nbins, "history": self.history, "words": self.buf.cpu().view(torch.int64).clone()}

    def load_state_dict(self, state):
        if (state["T"], state["nbins"], state["history"]) != (self.T, self.nbins, self.history):
            raise ValueError(f"LossBins: a state of T={state['T']} nbins={state['nbins']} history={state['history']} for bins of "
                             f"T={self.T} nbins={self.nbins} history={self.history}")
        self.buf.copy_(state["words"].view(torch.float64))


class DiffusionLoss:
    """`kind` "MSE" | "MAE" | "Huber" (torch's `nn.MSELoss` / `L1Loss` / `HuberLoss(delta)`, reduction "mean") with a per-image
    weight w_b = table[t_b] * sample_w[b]:  loss = mean_b w_b * mean_i l(pred - target)[b, i].  `table`: (T,) per-timestep
    weights (`min_snr_weights`) or None; `bins`: a `LossBins` that every call feeds with the UNWEIGHTED per-image losses, or None.
    Calls that produce a gradient also append to the bins' ring; calls under `torch.no_grad()` (validation) only add to sums
    and counts, so give them a `LossBins` of their own.
    A t outside [0, T) makes the loss NaN and is counted on the device; `check_faults()` raises for it."""

    def __init__(self, kind, table=None, bins=None, delta=1.0):
        if kind not in KINDS:
            raise ValueError("DiffusionLoss: kind must be MSE, MAE or Huber")
        if bins is not None and table is not None and table.numel() != bins.T:
            raise ValueError(f"DiffusionLoss: a table of {table.numel()} timesteps with bins of T={bins.T}")
        self.kind, self.delta, self.bins = kind, float(delta), bins
        self.table = None if table is None else table.detach().to(torch.float32).contiguous()
        self.per_image = None  # the last call's unweighted per-image losses, (B,) float64 on the device
        self.valid_counts = None  # the last call's valid pixels per image, (B,) int64 on the device; None without a mask
        self.loss_f64 = None   # the last call's loss before its rounding to fp32, 0-dim float64 on the device
        self._partials = self._bad_t = None

    def _launch(self, pred, target, t, sample_w, with_grad, valid=None):
        for name, x in (("pred", pred), ("target", target)):
            if not x.is_cuda or x.dtype != torch.float32:
                raise RuntimeError(f"DiffusionLoss: {name} must be an fp32 tensor on a ROCm device (there is no CPU path)")
        if pred.shape != target.shape or pred.dim() < 1:
            raise ValueError(f"DiffusionLoss: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        dev = pred.device
        pred, target = pred.detach().contiguous(), target.detach().contiguous()
        B = pred.shape[0]
        n = pred.numel() // max(B, 1)
        T = 0
        if self.table is not None or self.bins is not None:
            if t is None:
                raise ValueError("DiffusionLoss: a table or bins need the timesteps t")
            T = self.bins.T if self.bins is not None else self.table.numel()
            if self.table is not None and self.table.device != dev:
                self.table = self.table.to(dev)
            if self.bins is not None and self.bins.buf.device != dev:
                raise RuntimeError("DiffusionLoss: the bins live on another device")
        if t is not None:
            if not t.is_cuda or t.dtype != torch.int64 or t.numel() != B:
                raise RuntimeError(f"DiffusionLoss: t must be {B} int64 values on the device")
            t = t.contiguous()
        if sample_w is not None:
            if not sample_w.is_cuda or sample_w.dtype != torch.float32 or sample_w.numel() != B:
                raise RuntimeError(f"DiffusionLoss: sample_w must be {B} fp32 values on the device")
            sample_w = sample_w.contiguous()
        if valid is not None:
            if pred.dim() != 4:
                raise ValueError(f"DiffusionLoss: a mask needs pred as (B, C, H, W), got {tuple(pred.shape)}")
            if not valid.is_cuda or valid.dtype != torch.uint8 or valid.numel() * pred.shape[1] != pred.numel():
                raise RuntimeError(f"DiffusionLoss: valid must be {B} x {n // max(pred.shape[1], 1)} uint8 values on the device")
            valid = valid.contiguous()
        npart = B * ((n + 3) // CHUNK + 1)
        if self._partials is None or self._partials.numel() < npart or self._partials.device != dev:
            self._partials = torch.empty(npart, dtype=torch.float64, device=dev)
        if self._bad_t is None or self._bad_t.device != dev:
            self._bad_t = torch.zeros(1, dtype=torch.int64, device=dev)
        grad = torch.empty_like(pred) if with_grad else None
        self.per_image = torch.empty(B, dtype=torch.float64, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)  # the loss as double, and as fp32 in the first half of word 1
        bins = self.bins
        tail = (_ptr(out), _ptr(bins.buf if bins else None), bins.nbins if bins else 0, bins.history if bins else 0, int(with_grad),
                _ptr(self._bad_t), _stream(dev))
        self.valid_counts = None if valid is None else torch.empty(B, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            if valid is not None:
                entry = "drs_diffusion_loss_masked"
                st = _lib.load().drs_diffusion_loss_masked(
                    _ptr(pred), _ptr(target), _ptr(valid), _ptr(t), B, pred.shape[1], n // pred.shape[1], _ptr(self.table), T,
                    _ptr(sample_w), KINDS[self.kind], self.delta, _ptr(grad), _ptr(self.per_image), _ptr(self.valid_counts),
                    _ptr(self._partials), *tail)
            else:
                entry = "drs_diffusion_loss"
                st = _lib.load().drs_diffusion_loss(
                    _ptr(pred), _ptr(target), _ptr(t), B, n, _ptr(self.table), T, _ptr(sample_w), KINDS[self.kind], self.delta,
                    _ptr(grad), _ptr(self.per_image), _ptr(self._partials), *tail)
        _lib.check(st, entry)
        self.loss_f64 = out[0]
        return out.view(torch.float32)[2], grad

    def loss_and_grad(self, pred, target, t=None, sample_w=None, valid=None):
        """(loss, d loss / d pred) from the one launch: a 0-dim fp32 device tensor and a tensor of pred's shape, for
        `pred.backward(grad)`.  Appends to the bins' ring.  `valid`: (B, 1, H, W) uint8, non-zero = data (what
        `hip_ops.noise_target_nodata` returns): the loss over the valid pixels alone (include/drs_hip.h:
        drs_diffusion_loss_masked), each image's mean over its own valid elements, the batch mean over the images that have
        any; the gradient is +0.0 elsewhere and `valid_counts` holds the valid pixels per image.  None: the unmasked launch."""
        loss, grad = self._launch(pred, target, t, sample_w, True, **_masked(valid))
        return loss, grad.view(pred.shape)

    def __call__(self, pred, target, t=None, sample_w=None, valid=None):
        """The loss as a scalar that `.backward()` works on.  Under `torch.no_grad()`, or for a `pred` that needs no gradient, no
        gradient buffer is written and the ring is left alone."""
        if torch.is_grad_enabled() and pred.requires_grad:
            return _LossFunction.apply(pred, self, target, t, sample_w, valid)
        return self._launch(pred, target, t, sample_w, False, **_masked(valid))[0]

    def check_faults(self):
        """Raises if a call since the last check was handed a t outside [0, T).  Synchronises: for the end of an epoch."""
        bad = 0 if self._bad_t is None else int(self._bad_t.item())
        if bad:
            self._bad_t.zero_()
            raise RuntimeError(f"DiffusionLoss: {bad} timestep(s) outside [0, T) were handed to the loss; those images were "
                               "weighted with NaN and not binned")


class _LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, loss_fn, target, t, sample_w, valid=None):
        loss, grad = loss_fn._launch(pred, target, t, sample_w, True, **_masked(valid))
        ctx.save_for_backward(grad.view(pred.shape))
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return grad * grad_output, None, None, None, None, None


class LossAwareSampler:
    """Timesteps drawn on the device in proportion to sqrt(mean of the squared recent losses) of their bin, mixed with
    `eps_uniform` of the uniform distribution, and the importance weight that keeps the weighted loss an estimate of the uniform
    mean (`drs_timestep_draw`).  Uniform until every bin's ring is full.  Consumes the DEVICE generator (two `torch.rand` values
    per sample), not the CPU generator the uniform `Diffusion.sample_timesteps` draws from."""

    def __init__(self, bins, eps_uniform=1e-3):
        if not 0.0 <= eps_uniform <= 1.0:
            raise ValueError("LossAwareSampler: eps_uniform must lie in [0, 1]")
        self.bins, self.eps_uniform = bins, float(eps_uniform)

    def draw(self, B, u=None):
        """(t, sample_w): B int64 timesteps in 1 .. T - 1 and B fp32 weights, on the device, no synchronisation.  `u`: the
        (2, B) uniforms to use instead of drawing them."""
        dev = self.bins.buf.device
        if u is None:
            u = torch.rand(2, B, device=dev)
        elif u.shape != (2, B) or u.dtype != torch.float32 or u.device != dev:
            raise RuntimeError(f"LossAwareSampler: u must be (2, {B}) fp32 on the bins' device")
        u = u.contiguous()
        t = torch.empty(B, dtype=torch.int64, device=dev)
        w = torch.empty(B, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            st = _lib.load().drs_timestep_draw(_ptr(self.bins.buf), self.bins.nbins, self.bins.history, _ptr(u[0]), _ptr(u[1]),
                                               B, self.bins.T, self.eps_uniform, _ptr(t), _ptr(w), _stream(dev))
        _lib.check(st, "drs_timestep_draw")
        return t, w
