"""`optim.FusedAdamW` (csrc/optim.hip: drs_grad_sumsq_partials, drs_adamw_clip_multi) against the float64 oracle of
tests/optim_oracle.py, against `FusedAdam` bit for bit where they must agree, and the trainer's full resume."""
import copy
import math
import os
import shutil

import numpy as np
import pytest
import torch

from optim_oracle import AdamWOracle, global_norm

pytestmark = pytest.mark.gpu

NORM_SHAPES = [(1,), (5,), (4095,), (4096,), (4097,), (257, 100), (70001,), (32, 16, 3, 3)]  # chunk edges and a tail
RAGGED_SHAPES = [(32, 16, 3, 3), (5,), (1,), (257, 100), (3, 3, 3, 3), (70001,)]  # test_fused_adam_matches_torch_adam's
P_RTOL, P_ATOL, MOMENT_REL = 2e-6, 1e-7, 1e-6  # the project's Adam bars (test_gpu_parity.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _params(shapes, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    host = [torch.randn(s, generator=g) for s in shapes]
    return host, [torch.nn.Parameter(p.clone().to(dev)) for p in host]


def _ragged_grads(shapes, step, gen):
    """The gradients of step `step` of the ragged trajectory: tensor 2 never gets one, tensor 4 skips step 3."""
    return [None if i == 2 or (i == 4 and step == 3) else torch.randn(s, generator=gen) * (10.0 ** (step - 3))
            for i, s in enumerate(shapes)]


def _set_grads(params, grads, dev):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone().to(dev)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _assert_within_bars(opt, params, oracle, what=""):
    state = opt.state_dict()["state"]
    for i, p in enumerate(params):
        got, want = p.detach().cpu().double(), oracle.p[i]
        assert torch.allclose(got, want, rtol=P_RTOL, atol=P_ATOL), (what, i, (got - want).abs().max().item())
        if oracle.m[i] is None:
            assert i not in state
            continue
        assert float(state[i]["step"]) == oracle.steps[i]
        for name, ref in (("exp_avg", oracle.m[i]), ("exp_avg_sq", oracle.v[i])):
            err = (state[i][name].cpu().double() - ref).abs().max().item()
            assert err <= MOMENT_REL * ref.abs().max().item(), (what, i, name, err)


def _state_bits(opt, params):
    """Every parameter and moment as host copies, for bit comparisons."""
    out = [p.detach().cpu().clone() for p in params]
    for p in params:
        st = opt.state.get(p) or {}
        out += [st[k].cpu().clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


# ---- the norm ---------------------------------------------------------------------------------------------------------
def _norm_case(dev, big=None):
    from diffusionremotesensing_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(1)
    scales = np.logspace(-3, 3, len(NORM_SHAPES))
    grads = [torch.randn(s, generator=gen) * float(k) for s, k in zip(NORM_SHAPES, scales)]
    grads[3] = None  # one tensor without a gradient: its chunk contributes 0
    if big is not None:
        grads[big] = torch.full(NORM_SHAPES[big], 1e30)  # squares overflow fp32 and not double
    out = []
    for _ in range(2):
        _, params = _params(NORM_SHAPES, dev)
        opt = FusedAdamW(params, lr=0.0, max_grad_norm=1.0)
        _set_grads(params, grads, dev)
        opt.step()
        out.append((opt.last_grad_norm().cpu(), opt._partials.cpu().clone()))
    return grads, out


@pytest.mark.parametrize("big", [None, 5])
def test_global_norm_is_double_accurate_and_repeatable(dev, big):
    """Measured on MI355X: |norm - ref| / ref = 5.6e-9 and, with the 1e30 tensor, 1.5e-8, of the 1.19e-7 allowed."""
    grads, ((norm_a, part_a), (norm_b, part_b)) = _norm_case(dev, big)
    ref = global_norm(grads)
    assert math.isfinite(ref) and norm_a.dtype == torch.float32 and norm_a.dim() == 0
    err = abs(norm_a.double().item() - ref)
    print(f"norm {norm_a.item():.9g} ref {ref:.17g} err/ref {err / ref:.3e}")
    assert err <= 2.0 ** -23 * ref  # fp32 rounding of a double-accurate value, doubled
    assert torch.equal(norm_a, norm_b) and torch.equal(part_a, part_b)
    n_chunks = sum((int(np.prod(s)) + 4095) // 4096 for s in NORM_SHAPES)
    assert part_a.numel() == n_chunks
    # the partials themselves, chunk by chunk (float64 sums of at most 4096 squares: 1e-13 is far above their rounding)
    k = 0
    for s, g in zip(NORM_SHAPES, grads):
        n = int(np.prod(s))
        for lo in range(0, n, 4096):
            want = 0.0 if g is None else (g.reshape(-1)[lo:lo + 4096].double() ** 2).sum().item()
            assert abs(part_a[k].item() - want) <= 1e-13 * want, (s, lo)
            k += 1


# ---- trajectories -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm,weight_decay", [(1.0, 0.0), (0.05, 0.01), (None, 0.01)])
def test_trajectory_matches_the_float64_oracle(dev, max_norm, weight_decay):
    from diffusionremotesensing_amd.optim import FusedAdamW
    host, params = _params(RAGGED_SHAPES, dev)
    opt = FusedAdamW(params, lr=3e-4, weight_decay=weight_decay, max_grad_norm=max_norm)
    oracle = AdamWOracle(host, weight_decay=weight_decay, max_norm=max_norm)
    gen = torch.Generator().manual_seed(0)
    coefs = []
    for step in range(8):
        lr = 3e-4 * min(1.0, (step + 1) / 4)
        grads = _ragged_grads(RAGGED_SHAPES, step, gen)
        _set_grads(params, grads, dev)
        opt.param_groups[0]["lr"] = lr
        versions = [p._version for p in params]
        opt.step()
        assert all((p._version > v) == (g is not None) for p, v, g in zip(params, versions, grads))
        oracle.step(grads, lr)
        coefs.append((opt.last_clip_coef(), opt.last_grad_norm(), oracle.last_coef, oracle.last_norm))
    for step, (coef, norm, want_coef, want_norm) in enumerate(coefs):
        print(f"step {step}: coef {coef.item():.9g} oracle {want_coef:.9g} norm {norm.item():.9g} oracle {want_norm:.9g}")
        assert abs(coef.double().item() - want_coef) <= _ulp32(want_coef), step
        assert abs(norm.double().item() - want_norm) <= 2.0 ** -23 * want_norm, step
    _assert_within_bars(opt, params, oracle)
    assert opt.skipped_steps() == 0


@pytest.mark.parametrize("kwargs", [{}, {"max_grad_norm": 1e30}, {"skip_nonfinite": False}])
def test_without_clipping_and_decay_it_is_fused_adam_bit_for_bit(dev, kwargs):
    from diffusionremotesensing_amd.optim import FusedAdam, FusedAdamW
    _, a = _params(RAGGED_SHAPES, dev)
    _, b = _params(RAGGED_SHAPES, dev)
    plain, mine = FusedAdam(a, lr=3e-4), FusedAdamW(b, lr=3e-4, weight_decay=0.0, **kwargs)
    gen = torch.Generator().manual_seed(0)
    for step in range(6):
        grads = _ragged_grads(RAGGED_SHAPES, step, gen)
        _set_grads(a, grads, dev)
        _set_grads(b, grads, dev)
        plain.step()
        mine.step()
    bits_a, bits_b = _state_bits(plain, a), _state_bits(mine, b)
    assert len(bits_a) == len(bits_b) == 6 + 2 * 5
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(bits_a, bits_b))
    assert mine.last_clip_coef().item() == 1.0


# ---- the guard --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_step_is_skipped_on_the_device(dev, bad):
    from diffusionremotesensing_amd.optim import FusedAdamW
    host, params = _params(RAGGED_SHAPES, dev)
    opt = FusedAdamW(params, lr=3e-4, weight_decay=0.01, max_grad_norm=1.0)
    oracle = AdamWOracle(host, weight_decay=0.01, max_norm=1.0)
    gen = torch.Generator().manual_seed(0)
    for step in range(6):
        grads = _ragged_grads(RAGGED_SHAPES, step, gen)
        if step == 3:
            grads[5][40000] = bad  # one element, in the middle of a chunk of the largest tensor
        _set_grads(params, grads, dev)
        before = _state_bits(opt, params)
        opt.step()
        oracle.step(grads, 3e-4)
        if step == 3:
            after = _state_bits(opt, params)
            assert len(before) == len(after)
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, after))
            assert not math.isfinite(opt.last_grad_norm().item())
    assert opt.skipped_steps() == 1 == oracle.skipped
    _assert_within_bars(opt, params, oracle, "after the skipped step")


def test_no_norm_launch_without_clipping_and_guard(dev, monkeypatch):
    """Counted at the binding (the library's launch log covers only a plan's profiled forward, not the plan-less entry points)."""
    from diffusionremotesensing_amd import _lib
    from diffusionremotesensing_amd.optim import FusedAdamW
    lib = _lib.load()
    calls = {"norm": 0, "update": 0}
    norm_fn, update_fn = lib.drs_grad_sumsq_partials, lib.drs_adamw_clip_multi
    monkeypatch.setattr(lib, "drs_grad_sumsq_partials", lambda *a: calls.__setitem__("norm", calls["norm"] + 1) or norm_fn(*a))
    monkeypatch.setattr(lib, "drs_adamw_clip_multi", lambda *a: calls.__setitem__("update", calls["update"] + 1) or update_fn(*a))
    host, params = _params(RAGGED_SHAPES, dev)
    oracle = AdamWOracle(host, weight_decay=0.01, skip_nonfinite=False)
    gen = torch.Generator().manual_seed(0)
    grads = _ragged_grads(RAGGED_SHAPES, 3, gen)
    _set_grads(params, grads, dev)
    opt = FusedAdamW(params, lr=3e-4, weight_decay=0.01, skip_nonfinite=False)
    opt.step()
    oracle.step(grads, 3e-4)
    assert calls == {"norm": 0, "update": 1}
    _assert_within_bars(opt, params, oracle)
    FusedAdamW(params, lr=3e-4, max_grad_norm=1.0).step()
    assert calls == {"norm": 1, "update": 2}


# ---- ordering ---------------------------------------------------------------------------------------------------------
def test_norm_is_taken_after_grad_ready(dev):
    """`grad_ready` writes the gradients in place (what the wait of the gradient exchange does): norm and update must be the
    oracle's for the written gradients, not for what the buffers held when the table was built."""
    from diffusionremotesensing_amd.optim import FusedAdamW
    shapes = [s for i, s in enumerate(RAGGED_SHAPES) if i != 2]
    host, params = _params(shapes, dev)
    opt = FusedAdamW(params, lr=3e-4, weight_decay=0.01, max_grad_norm=0.5)
    oracle = AdamWOracle(host, weight_decay=0.01, max_norm=0.5)
    gen = torch.Generator().manual_seed(3)
    for step in range(2):
        grads = [torch.randn(s, generator=gen) for s in shapes]
        for p in params:
            p.grad = torch.full_like(p, 1e6)
        staged = [g.to(dev) for g in grads]

        def ready():
            for p, g in zip(params, staged):
                p.grad.copy_(g)
        opt.step(grad_ready=ready)
        oracle.step(grads, 3e-4)
        assert abs(opt.last_grad_norm().double().item() - oracle.last_norm) <= 2.0 ** -23 * oracle.last_norm
    _assert_within_bars(opt, params, oracle)


# ---- the trainer ------------------------------------------------------------------------------------------------------
TRAIN_KWARGS = dict(lr=1e-3, check_preds_epoch=1, val_loader=None, patience=5, loss="MSE", verbose=False, weight_decay=0.01,
                    max_grad_norm=1.0, lr_schedule="cosine", warmup_steps=2, save_train_state=True)


class _Interrupt(Exception):
    pass


class _StopAfter:
    """The loader, until its epoch number `epochs` is asked for: the run dies there, after the snapshot of the epoch before."""

    def __init__(self, loader, epochs):
        self.loader, self.left = loader, epochs

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if self.left == 0:
            raise _Interrupt
        self.left -= 1
        return iter(self.loader)


def _run(dev, seeded_sd, folder, epochs, stop_after=None, seed=True):
    """test_diffusion_train_loop_end_to_end's configuration (image 32, T = 50, 8 synthetic images in batches of 4, EMA) with
    clipping, decay, a cosine schedule and the sidecar; every epoch saves."""
    from torch.utils.data import DataLoader
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion, SyntheticSuperresDataset
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    if seed:
        torch.manual_seed(0)
        torch.cuda.manual_seed(0)
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev)
    d = Diffusion("cosine", m, os.path.join(folder, "snapshot.pt"), noise_steps=50, device=dev, magnification_factor=2,
                  image_size=32, Degradation_type="DownBlur", ema_smoothing=True)
    loader = DataLoader(SyntheticSuperresDataset(8, 3, 32, 2, seed=5), batch_size=4, shuffle=False)
    if stop_after is not None:
        with pytest.raises(_Interrupt):
            d.train(epochs=epochs, train_loader=_StopAfter(loader, stop_after), **TRAIN_KWARGS)
    else:
        d.train(epochs=epochs, train_loader=loader, **TRAIN_KWARGS)
    return d


@pytest.fixture(scope="module")
def two_epochs(dev, seeded_sd, tmp_path_factory):
    folder = str(tmp_path_factory.mktemp("run2"))
    d = _run(dev, seeded_sd, folder, 2)
    return folder, d, torch.get_rng_state(), torch.cuda.get_rng_state(dev)


def _equal_state_dicts(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_sidecar_restores_the_whole_training_state(dev, seeded_sd, two_epochs):
    folder, d, cpu_rng, dev_rng = two_epochs
    snap = torch.load(os.path.join(folder, "snapshot.pt"))
    assert set(snap) == {"MODEL_STATE", "EPOCHS_RUN"} and len(snap["MODEL_STATE"]) == 299 and snap["EPOCHS_RUN"] == 1
    assert sorted(os.listdir(folder)) == ["snapshot.pt", "train_state.pt"]
    ts = torch.load(os.path.join(folder, "train_state.pt"))
    assert ts["NEXT_EPOCH"] == 2 and ts["EMA_STEP"] == 4 and ts["LR_SCHEDULE"]["last_step"] == 4
    # a fresh model and Diffusion, restored from the two files (epochs=2: nothing is left to train)
    torch.manual_seed(99)
    torch.cuda.manual_seed(99)
    d2 = _run(dev, seeded_sd, folder, 2, seed=False)
    a, b = d.train_state, d2.train_state
    assert d2.epochs_run == 2 and type(a.optimizer) is type(b.optimizer)
    sa, sb = a.optimizer.state_dict(), b.optimizer.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and set(sa["state"]) == set(sb["state"]) and len(sa["state"]) > 100
    for k in sa["state"]:
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 4.0
        assert all(torch.equal(sa["state"][k][n], sb["state"][k][n]) for n in ("exp_avg", "exp_avg_sq"))
    assert _equal_state_dicts(d.model.state_dict(), d2.model.state_dict())            # raw weights
    assert _equal_state_dicts(a.ema_model.state_dict(), b.ema_model.state_dict())    # the snapshot's
    assert _equal_state_dicts(b.ema_model.state_dict(), {k: v.to(dev) for k, v in snap["MODEL_STATE"].items()})
    assert a.ema.step == b.ema.step == 4
    assert a.scheduler.state_dict() == b.scheduler.state_dict() and b.scheduler.last_step == 4
    assert a.best_loss == b.best_loss and a.epochs_without_improving == b.epochs_without_improving == 0
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(dev), dev_rng)
    assert b.optimizer.skipped_steps() == 0


def test_mismatched_sidecar_raises(dev, seeded_sd, two_epochs, tmp_path):
    folder = two_epochs[0]
    for name in ("snapshot.pt", "train_state.pt"):
        shutil.copy(os.path.join(folder, name), tmp_path / name)
    ts = torch.load(tmp_path / "train_state.pt")
    other = copy.deepcopy(ts)
    last = other["OPTIMIZER_STATE"]["param_groups"][0]["params"].pop()  # one parameter fewer
    other["OPTIMIZER_STATE"]["state"].pop(last, None)
    torch.save(other, tmp_path / "train_state.pt")
    with pytest.raises(ValueError):
        _run(dev, seeded_sd, str(tmp_path), 2)
    other = copy.deepcopy(ts)
    st = other["OPTIMIZER_STATE"]["state"][0]
    st["exp_avg"] = st["exp_avg"].reshape(-1)[:-1].clone()  # another shape
    torch.save(other, tmp_path / "train_state.pt")
    with pytest.raises(ValueError):
        _run(dev, seeded_sd, str(tmp_path), 2)


def _max_abs_diff(a, b):
    return max((p.detach() - q.detach()).abs().max().item() for p, q in zip(a.model.parameters(), b.model.parameters()))


def test_resumed_run_continues_like_the_uninterrupted_one(dev, seeded_sd, tmp_path):
    """A: 4 epochs.  A': the same again.  B: the same run killed after 2 epochs and started again.  d_AB <= 4 * d_AA, which is
    equality where a training step is bit-repeatable.  Measured on MI355X in two sessions: d_AA 1.41e-3 / 1.61e-3, d_AB 1.66e-3 /
    2.55e-3, of 5.04e-3 that the run moves the weights (a step here is not bit-repeatable)."""
    runs = {}
    for name in ("A", "A2", "B"):
        os.makedirs(tmp_path / name)
    runs["A"] = _run(dev, seeded_sd, str(tmp_path / "A"), 4)
    runs["A2"] = _run(dev, seeded_sd, str(tmp_path / "A2"), 4)
    _run(dev, seeded_sd, str(tmp_path / "B"), 4, stop_after=2)
    assert torch.load(tmp_path / "B" / "train_state.pt")["NEXT_EPOCH"] == 2
    torch.manual_seed(7)  # the restart is another process: its generators start elsewhere
    torch.cuda.manual_seed(7)
    runs["B"] = _run(dev, seeded_sd, str(tmp_path / "B"), 4, seed=False)
    assert runs["B"].train_state.ema.step == runs["A"].train_state.ema.step == 8
    assert torch.load(tmp_path / "B" / "train_state.pt")["NEXT_EPOCH"] == 4
    d_aa, d_ab = _max_abs_diff(runs["A"], runs["A2"]), _max_abs_diff(runs["A"], runs["B"])
    moved = _max_abs_diff(runs["A"], _untrained(dev, seeded_sd))
    print(f"d_AA {d_aa:.3e} d_AB {d_ab:.3e} (the run moved the weights by up to {moved:.3e})")
    assert moved > 1e-4  # the four epochs did train
    assert d_ab <= 4 * d_aa


def _untrained(dev, seeded_sd):
    """The untrained model as a stand-in with `.model`, for `_max_abs_diff`."""
    import types
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    return types.SimpleNamespace(model=m.to(dev))
