"""`FusedAdam`: torch.optim.Adam's update (defaults of the reference: `Adam(model.parameters(), lr=lr)`,
train_diffusion_superres.py:337) as ONE multi-tensor HIP launch per step (`drs_adam_multi`) instead of the ~45
foreach kernels torch issues for the UNet's 176 parameter tensors.

Same `state_dict()` layout as torch.optim.Adam (`step`, `exp_avg`, `exp_avg_sq` per parameter), same treatment of
parameters without a gradient (skipped, state untouched).  Parameters must be fp32 tensors on a ROCm device.

`FusedAdamW`: the same with decoupled weight decay, clipping of the global gradient norm and a guard against non-finite
gradients (`drs_grad_sumsq_partials` + `drs_adamw_clip_multi`, no host synchronisation); `WarmupCosine`: the learning-rate
schedule that goes with it.  Both are off in a default training run.
"""
import ctypes as C

import torch

from . import _lib


class _AdamTensor(C.Structure):  # include/drs_hip.h: drs_adam_tensor
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("step", C.c_int64)]


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("FusedAdam: invalid hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self._tables = {}

    @torch.no_grad()
    def step(self, closure=None, grad_ready=None):
        """`grad_ready`, when given, is called after the host-side table build and right before the update kernel is
        enqueued: the multi-GPU step passes the wait of its asynchronous gradient all-reduce, so the collective overlaps
        the table build (`dist.allreduce_gradients(async_op=True)`).  Gradients that are None at call time but may be
        produced by that wait (parameters unused on this rank only) are resolved first."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_ready = self._wait_first_if_needed(grad_ready)
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            dev = params[0].device
            rows, live = self._rows(params)
            if not live:
                continue
            devt = self._upload(gi, rows, dev)
            b1, b2 = group["betas"]
            if grad_ready is not None:
                self._late_wait(grad_ready)
                grad_ready = None
            with torch.cuda.device(dev):
                st = lib.drs_adam_multi(C.c_void_p(devt.data_ptr()), len(rows), max(r[4] for r in rows), float(group["lr"]),
                                        float(b1), float(b2), float(group["eps"]),
                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            _lib.check(st, "drs_adam_multi")
            # the kernel wrote the parameters through raw pointers: advance their version counters (no kernel launch) so
            # that everything keyed on `_version` (the engine's packed-weight cache) sees the update
            torch.autograd.graph.increment_version([p for p in params if p.grad is not None])
        if grad_ready is not None:
            self._late_wait(grad_ready)
        return loss

    def _wait_first_if_needed(self, grad_ready):
        """Runs `grad_ready` now, and returns None, when which gradients exist is only known after the exchange."""
        owner = getattr(grad_ready, "__self__", None) if grad_ready is not None else None
        has_flag_tail = owner is not None and hasattr(owner, "flat") and owner.flat.numel() > getattr(owner, "n_grad", 0)
        if grad_ready is not None and (has_flag_tail or any(p.grad is None and getattr(p, "_drs_maybe_unused", False)
                                                            for g in self.param_groups for p in g["params"])):
            # which gradients exist is only known after the exchange: whenever it carries "used" flags (some parameter may be
            # unused on some rank) it is waited for BEFORE any table is built - on every rank alike, so no rank can end up
            # with a gradient that has no row (the condition _late_wait still checks, now unreachable through dist.py)
            grad_ready()
            grad_ready = None
        return grad_ready

    def _rows(self, params):
        """(rows (p, g, m, v, n, step) of one group's table - g = 0 for a parameter without a gradient -, whether any has one);
        creates the state of a parameter at its first gradient and counts its step."""
        rows, live = [], False
        for p in params:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("FusedAdam: parameters must be contiguous fp32 tensors on a ROCm device")
            if p.grad is None:  # no state is created for a parameter that never gets a gradient (like torch)
                rows.append((p.data_ptr(), 0, 0, 0, p.numel(), 0))
                continue
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["step"] += 1
            s = int(st["step"].item())  # host tensor: no device sync
            g = p.grad
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
                p.grad = g
            rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), s))
            live = True
        return rows, live

    def _upload(self, gi, rows, dev):
        """The device copy of group `gi`'s pointer table: the gradients move every step (fresh flat buffer per backward), so the
        table is uploaded each step from a small ring of pinned buffers; a slot is reused only after its copy has executed."""
        size = len(rows) * len(rows[0])
        ring = self._tables.get(gi)
        if ring is None or ring["dev"].numel() != size:
            ring = {"host": [torch.empty(size, dtype=torch.int64).pin_memory() for _ in range(4)],
                    "event": [None] * 4, "dev": torch.empty(size, dtype=torch.int64, device=dev), "k": 0}
            self._tables[gi] = ring
        k = ring["k"]
        ring["k"] = (k + 1) % 4
        if ring["event"][k] is not None:
            ring["event"][k].synchronize()
        host, devt = ring["host"][k], ring["dev"]
        host.copy_(torch.tensor(rows, dtype=torch.int64).view(-1))
        devt.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        ring["event"][k] = ev
        return devt

    @staticmethod
    def _late_wait(grad_ready):
        """The exchange's wait, AFTER the pointer table was built.  A gradient that the wait itself creates (parameter unused
        on this rank, used on another: dist._PendingReduce.created_grads) has no row in that table: this rank would skip the
        update the other ranks apply and the replicas would drift apart silently.  Parameters that can be unused per rank
        must carry `_drs_maybe_unused` (then the wait runs first); anything else is reported, not ignored."""
        grad_ready()
        owner = getattr(grad_ready, "__self__", None)
        created = getattr(owner, "created_grads", None)
        if created:
            raise RuntimeError(f"FusedAdam: the gradient exchange created .grad for {len(created)} parameter(s) after the "
                               "update table was built; mark parameters that may be unused on some ranks with "
                               "`p._drs_maybe_unused = True` so that the exchange is waited for first")


class _AdamWTensor(C.Structure):  # include/drs_hip.h: drs_adamw_tensor
    _fields_ = _AdamTensor._fields_ + [("part0", C.c_int64)]


CHUNK = 4096  # elements per block of the multi-tensor kernels (csrc/optim.hip): one partial sum of squares per chunk


class FusedAdamW(FusedAdam):
    """`FusedAdam` with decoupled weight decay (torch.optim.AdamW's `param.mul_(1 - lr * weight_decay)`), clipping of the
    GLOBAL gradient norm (torch.nn.utils.clip_grad_norm_ over every parameter of every group, `max_grad_norm`; None = off) and
    a guard that skips the whole step when that norm is not finite (`skip_nonfinite`) - two launches per group and step
    (`drs_grad_sumsq_partials`, `drs_adamw_clip_multi`) and no host synchronisation: the update kernel reads the norm on the
    device.  With neither clipping nor the guard there is no norm launch.

    A skipped step leaves parameters and moments untouched, but the per-parameter `step` of the state counts it (the host does
    not know): bias correction is one step ahead after a skip.  With weight_decay == 0 and no clipping the update is bit for
    bit `FusedAdam`'s.  All parameters must live on one device."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=None,
                 skip_nonfinite=True):
        if weight_decay < 0 or (max_grad_norm is not None and not max_grad_norm > 0):
            raise ValueError("FusedAdamW: invalid hyper-parameters")
        super().__init__(params, lr=lr, betas=betas, eps=eps)
        for group in self.param_groups:
            group.setdefault("weight_decay", weight_decay)
        self.defaults["weight_decay"] = weight_decay
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        self._partials = None
        self._stats = None  # drs_adamw_stats as six int32 words: norm, coef, skipped, -, skipped_total (two words)

    def _device_stats(self, dev):
        if self._stats is None:
            self._stats = torch.zeros(6, dtype=torch.int32, device=dev)
        return self._stats

    @torch.no_grad()
    def step(self, closure=None, grad_ready=None):
        """`grad_ready` as in `FusedAdam.step`; it has returned before the norm launch is enqueued, so under --multiple_gpus
        the norm is that of the averaged gradients, the same on every rank."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        grad_ready = self._wait_first_if_needed(grad_ready)
        tables, part0, dev = [], 0, None
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            if dev is not None and params[0].device != dev:
                raise RuntimeError("FusedAdamW: the global gradient norm needs all parameters on one device")
            dev = params[0].device
            rows, live = self._rows(params)
            if not live:
                continue
            for i, r in enumerate(rows):  # every tensor owns one partial per chunk, back to back over all groups
                rows[i] = r + (part0,)
                part0 += (r[4] + CHUNK - 1) // CHUNK
            tables.append((group, rows, self._upload(gi, rows, dev)))
        if grad_ready is not None:
            self._late_wait(grad_ready)
        if not tables:
            return loss
        with_norm = self.max_grad_norm is not None or self.skip_nonfinite
        npartials = part0 if with_norm else 0
        if with_norm and (self._partials is None or self._partials.numel() < npartials):
            self._partials = torch.empty(npartials, dtype=torch.float64, device=dev)
        partials = C.c_void_p(self._partials.data_ptr()) if with_norm else None
        stats = self._device_stats(dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if with_norm:
                for _, rows, devt in tables:
                    _lib.check(lib.drs_grad_sumsq_partials(C.c_void_p(devt.data_ptr()), len(rows), max(r[4] for r in rows),
                                                           partials, stream), "drs_grad_sumsq_partials")
            for k, (group, rows, devt) in enumerate(tables):
                b1, b2 = group["betas"]
                st = lib.drs_adamw_clip_multi(C.c_void_p(devt.data_ptr()), len(rows), max(r[4] for r in rows),
                                              float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                              float(group["weight_decay"]), float(self.max_grad_norm or 0.0),
                                              int(self.skip_nonfinite), partials, npartials,
                                              C.c_void_p(stats.data_ptr()) if k == 0 else None, stream)
                _lib.check(st, "drs_adamw_clip_multi")
        for group, _, _ in tables:  # (see FusedAdam.step: the kernels wrote through raw pointers)
            torch.autograd.graph.increment_version([p for p in group["params"] if p.grad is not None])
        return loss

    def _stat(self, dtype, index):
        if self._stats is None:
            raise RuntimeError("FusedAdamW: no step has run yet")
        return self._stats.view(dtype)[index].clone()

    def last_grad_norm(self):
        """The last step's global gradient norm BEFORE clipping, a 0-dim fp32 device tensor (no synchronisation); 0 when
        neither clipping nor the guard is on (the norm is not computed then)."""
        return self._stat(torch.float32, 0)

    def last_clip_coef(self):
        """The factor the last step's gradients were multiplied by, a 0-dim fp32 device tensor (no synchronisation)."""
        return self._stat(torch.float32, 1)

    def skipped_steps(self):
        """How many steps the non-finite guard has skipped so far.  Synchronises: for the end of an epoch."""
        return 0 if self._stats is None else int(self._stats.view(torch.int64)[2].item())

    def load_state_dict(self, state_dict):
        """State of `FusedAdam`, `FusedAdamW` or `torch.optim.Adam[W]` (same per-parameter layout): the saved groups'
        hyper-parameters are taken as torch does, those they lack keep this optimizer's; `step` goes to the host.  A state
        whose parameter count or tensor shapes differ from this optimizer's parameters raises ValueError."""
        mine = {k: v for k, v in self.defaults.items()}
        own_groups = [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, own in zip(self.param_groups, own_groups):
            for k, v in {**mine, **own}.items():
                group.setdefault(k, v)
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                for name in ("exp_avg", "exp_avg_sq"):
                    if name not in st or st[name].shape != p.shape:
                        raise ValueError(f"FusedAdamW.load_state_dict: {name} of shape "
                                         f"{tuple(st[name].shape) if name in st else None} for a parameter of shape "
                                         f"{tuple(p.shape)}")
                    st[name] = st[name].to(device=p.device, dtype=torch.float32).contiguous()
                st["step"] = torch.as_tensor(st["step"]).detach().to("cpu", torch.float32).reshape(())
        self._tables = {}


class WarmupCosine:
    """Learning rate by global optimizer step s = 0, 1, ...: linear from base_lr / warmup_steps (s = 0) to base_lr
    (s = warmup_steps - 1), then - `kind="cosine"` - half a cosine from base_lr at s = warmup_steps down to lr_min at
    s = total_steps (and lr_min after it), or - `kind="constant"` - base_lr.  `step(optimizer)` writes the current step's rate
    into every group's "lr" and moves on: call it right before `optimizer.step()` (the kernels take lr per launch)."""

    def __init__(self, base_lr, warmup_steps=0, total_steps=0, lr_min=0.0, kind="cosine"):
        if kind not in ("constant", "cosine"):
            raise ValueError("WarmupCosine: kind must be constant or cosine")
        if base_lr < 0 or lr_min < 0 or warmup_steps < 0 or (kind == "cosine" and total_steps <= warmup_steps):
            raise ValueError("WarmupCosine: need base_lr, lr_min, warmup_steps >= 0 and total_steps > warmup_steps")
        self.base_lr, self.warmup_steps, self.total_steps = float(base_lr), int(warmup_steps), int(total_steps)
        self.lr_min, self.kind = float(lr_min), kind
        self.last_step = 0  # the step the next `step()` call sets the rate of

    def lr_at(self, s):
        import math
        if s < self.warmup_steps:
            return self.base_lr * (s + 1) / self.warmup_steps
        if self.kind == "constant":
            return self.base_lr
        x = min(1.0, (s - self.warmup_steps) / (self.total_steps - self.warmup_steps))
        return self.lr_min + (self.base_lr - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * x))

    def step(self, optimizer):
        lr = self.lr_at(self.last_step)
        for group in optimizer.param_groups:
            group["lr"] = lr
        self.last_step += 1
        return lr

    def state_dict(self):
        return dict(vars(self))

    def load_state_dict(self, state):
        for k in vars(self):
            setattr(self, k, state[k])
