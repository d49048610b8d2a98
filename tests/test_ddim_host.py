"""DDIM sampling without a GPU: the timestep list, the float64 oracle against the reference's ancestral arithmetic, the
chain loop on list positions (fault hand-over), argument checks of Diffusion.sample and drs_ddim_step, and the CLI flags."""
import ctypes as C
import math

import pytest
import torch

import ddim_oracle as O
from oracle import diffusion_oracle as D


# ---------------------------------------------------------------------------------------------
# timestep list
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 3, 50, 1000, 1500])
def test_ddim_timesteps(T):
    from diffusionremotesensing_amd.train_diffusion_superres import ddim_timesteps
    assert ddim_timesteps(T, 1) == [T - 1]
    assert ddim_timesteps(T, T - 1) == list(range(T - 1, 0, -1))  # the ancestral chain's timesteps
    for S in sorted({1, 2, 5, 25, 50, T // 2, T - 2, T - 1}):
        if not 1 <= S <= T - 1:
            continue
        ts = ddim_timesteps(T, S)
        assert len(ts) == S and all(type(t) is int for t in ts)
        assert all(a > b for a, b in zip(ts, ts[1:]))  # strictly descending, hence unique
        assert ts[0] == T - 1 and (ts[-1] == 1 or S == 1)
        assert ts == O.timesteps(T, S)
    if T >= 3:
        assert ddim_timesteps(T, 2) == [T - 1, 1]
    for S in (0, -1, T, T + 5):
        with pytest.raises(ValueError):
            ddim_timesteps(T, S)


def test_ddim_timesteps_known_values():
    from diffusionremotesensing_amd.train_diffusion_superres import ddim_timesteps
    assert ddim_timesteps(50, 7) == [49, 41, 33, 25, 17, 9, 1]
    ts = ddim_timesteps(1500, 50)
    assert ts[:3] == [1499, 1468, 1437] and ts[-2:] == [31, 1]


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
def _schedule64(kind, T):
    """(alpha, alpha_hat, beta) in float64 with alpha_t = alpha_hat_t / alpha_hat_{t-1} exactly (t >= 1)."""
    if kind == "linear":
        alpha = 1.0 - torch.linspace(1e-4, 0.02, T, dtype=torch.float64)
        ah = torch.cumprod(alpha, 0)
    else:
        ah = D.cosine_alpha_hat(T).double()
    beta = torch.empty_like(ah)
    beta[0] = 1 - ah[0]
    beta[1:] = 1 - ah[1:] / ah[:-1]
    return 1 - beta, ah, beta


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_oracle_eta1_single_step_is_the_ancestral_step(kind):
    """eta = 1 from t to t - 1: sigma^2 is the posterior variance beta~_t = (1 - ah_{t-1}) / (1 - ah_t) * beta_t, and the
    mean is the reference's 1/sqrt(a) (x - (1 - a)/sqrt(1 - ah) eps): the reference's update with z scaled by
    sqrt(beta~_t / beta_t)."""
    T = 1000
    a, ah, b = _schedule64(kind, T)
    g = torch.Generator().manual_seed(3)
    x, e, z = (torch.randn((2, 3, 4, 4), generator=g, dtype=torch.float64) for _ in range(3))
    for t in (2, 3, 17, 250, 500, 998, 999):
        bt = (1 - ah[t - 1]) / (1 - ah[t]) * b[t]
        want = D.sampler_step(x, e, z * torch.sqrt(bt / b[t]), torch.full((2,), t, dtype=torch.long), a, ah, b)
        got = O.step(x, e, z, t, t - 1, 1.0, ah)
        assert torch.allclose(got, want, rtol=1e-11, atol=1e-11 * want.abs().max().item()), (kind, t)
    # the last move (to t = 0) adds no noise whatever eta is, as the reference adds zeros at its last step; for the cosine
    # schedule (alpha_hat[0] = 1) both updates are then the x0 prediction (x - sqrt(1 - ah_1) eps) / sqrt(ah_1)
    assert O.coefficients(1, 0, 1.0, ah)[2] == 0.0
    if kind == "cosine":
        want = D.sampler_step(x, e, torch.zeros_like(x), torch.ones(2, dtype=torch.long), a, ah, b)
        assert torch.allclose(O.step(x, e, None, 1, 0, 1.0, ah), want, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("S", [1, 5, 1499])
def test_oracle_eta0_chain_recovers_x0(S):
    """With the eps a perfect model predicts for a known x0, eps = (x_t - sqrt(ah_t) x0) / sqrt(1 - ah_t), the deterministic
    chain lands on x0 (cosine: alpha_hat[0] = 1)."""
    T = 1500
    _, ah, _ = D.schedule("cosine", T)
    assert float(ah[0]) == 1.0
    g = torch.Generator().manual_seed(7)
    x0 = torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64) * 2 - 1
    xT = torch.randn((2, 3, 8, 8), generator=g, dtype=torch.float64)

    taus = O.timesteps(T, S)
    x = xT.clone()
    for k, t in enumerate(taus):
        tp = taus[k + 1] if k + 1 < len(taus) else 0
        at = float(ah[t])
        eps = (x - math.sqrt(at) * x0) / math.sqrt(1 - at)
        x = O.step(x, eps, None, t, tp, 0.0, ah)
    err = (x - x0).abs().max().item()
    assert err <= 1e-11, err


def test_oracle_chain_noise_protocol():
    """x_T comes from noise_source(T, .); with eta = 0 nothing else is drawn; with eta > 0 every move but the last draws
    once, keyed by the timestep it leaves."""
    _, ah, _ = D.schedule("cosine", 50)
    for eta, want in ((0.0, [50]), (0.5, [50, 49, 41, 33, 25, 17, 9])):
        calls = []

        def src(i, shape):
            calls.append(i)
            return torch.zeros(shape)
        O.chain(lambda x, t: torch.zeros_like(x), (1, 1, 2, 2), 50, ah, 7, eta, src)
        assert calls == want


# ---------------------------------------------------------------------------------------------
# the chain loop on list positions
# ---------------------------------------------------------------------------------------------
class _FaultOnce:
    def __init__(self, fail_at):
        self.calls, self.fail_at = 0, fail_at

    def check_faults(self):
        self.calls += 1
        if self.calls == self.fail_at:
            from diffusionremotesensing_amd import _lib
            raise _lib.RangeFault("drs_unet_check_faults failed with status 6: test")


def test_run_reverse_chain_with_a_list_resumes_at_the_checkpoint_position(capsys):
    from diffusionremotesensing_amd.train_diffusion_superres import ddim_timesteps, run_reverse_chain
    taus = ddim_timesteps(100, 10)  # [99, 88, 77, 67, 56, 45, 34, 23, 12, 1]
    x = torch.zeros(1)
    seen, frames = [], []

    def step(i):
        seen.append(i)
        x.add_(i)
        frames.append(i)
    eng = _FaultOnce(fail_at=2)  # the check after positions 4..7 raises once
    run_reverse_chain(eng, x, 100, step, frames, every=4, timesteps=taus)
    assert seen == taus[:8] + taus[4:8] + taus[8:]
    assert frames == taus  # the frames of the rolled-back steps were dropped
    assert x.item() == sum(taus)  # x went back to its checkpoint before positions 4..7 ran again
    assert eng.calls == 4  # after 4, after 8 (fault), after 8 again, at the end
    assert f"resuming the chain at step {taus[4]}" in capsys.readouterr().err


def test_run_reverse_chain_fault_at_the_final_check():
    from diffusionremotesensing_amd.train_diffusion_superres import run_reverse_chain
    taus = [40, 30, 20, 10, 1]
    x = torch.zeros(1)
    seen = []

    def step(i):
        seen.append(i)
        x.add_(1)
    eng = _FaultOnce(fail_at=2)
    run_reverse_chain(eng, x, 41, step, None, every=3, timesteps=taus)
    assert seen == [40, 30, 20, 10, 1, 10, 1] and x.item() == 5


def test_run_reverse_chain_without_a_list_visits_every_timestep():
    from diffusionremotesensing_amd.train_diffusion_superres import run_reverse_chain
    seen = []
    run_reverse_chain(_FaultOnce(fail_at=0), torch.zeros(1), 50, seen.append, None, every=7)
    assert seen == list(range(49, 0, -1))
    seen.clear()
    eng = _FaultOnce(fail_at=3)
    run_reverse_chain(eng, torch.zeros(1), 30, seen.append, None, every=10)
    assert seen == list(range(29, 0, -1)) + list(range(9, 0, -1))  # last block (9 .. 1) re-run
    assert eng.calls == 4


# ---------------------------------------------------------------------------------------------
# argument checks (no engine, no GPU)
# ---------------------------------------------------------------------------------------------
def test_diffusion_sample_rejects_bad_ddim_arguments():
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as GenDiffusion
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as SarDiffusion
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion

    class NoEngine(torch.nn.Module):
        def hip_engine(self):
            raise AssertionError("the engine must not be touched before the arguments are checked")

    T = 20
    m = NoEngine()
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device="cpu", magnification_factor=2,
                  image_size=16, Degradation_type="DownBlur")
    ds = SarDiffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device="cpu", image_size=16)
    dg = GenDiffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device="cpu", image_size=16)
    calls = [lambda **kw: d.sample(1, m, torch.zeros(3, 8, 8), **kw),
             lambda **kw: ds.sample(1, m, torch.zeros(2, 16, 16), **kw),
             lambda **kw: dg.sample(1, m, target_class=torch.tensor([1]), **kw)]
    for call in calls:
        for kw in ({"sampling_steps": 0}, {"sampling_steps": T}, {"sampling_steps": -1}, {"sampling_steps": 2.5},
                   {"sampling_steps": 5, "eta": -0.1}, {"sampling_steps": 5, "eta": float("nan")}):
            with pytest.raises(ValueError):
                call(**kw)
        with pytest.raises(AssertionError, match="engine"):  # valid arguments get as far as the engine
            call(sampling_steps=T - 1, eta=1.0)


def test_ddim_step_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 16)()  # host memory: every call below must fail validation before any launch
    p = C.cast(buf, C.c_void_p)

    def call(x=p, ec=p, eu=None, w=0.0, z=p, t=10, tp=5, eta=0.5, ah=p, T=50, n=16):
        return lib.drs_ddim_step(x, ec, eu, w, z, t, tp, eta, ah, T, n, None)

    for kw, msg in (({"x": None}, b"null pointer"), ({"ec": None}, b"null pointer"), ({"ah": None}, b"null pointer"),
                    ({"tp": 10}, b"t_prev"), ({"tp": 11}, b"t_prev"), ({"tp": -1}, b"t_prev"), ({"t": 50}, b"t_prev"),
                    ({"eta": -0.1}, b"eta"), ({"eta": float("nan")}, b"eta"), ({"eta": float("inf")}, b"eta"),
                    ({"z": None}, b"noise")):
        assert call(**kw) == 1, kw
        assert msg in lib.drs_last_error(), (kw, lib.drs_last_error())


def test_ddim_step_wrapper_has_no_cpu_fallback():
    from diffusionremotesensing_amd import hip_ops
    x = torch.zeros(4)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.ddim_step_(x, x, None, 10, 5, 0.0, torch.ones(50))


# ---------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------
def test_sampling_flags_on_every_parser():
    from diffusionremotesensing_amd import Aggregation_Sampling, train_diffusion_SAR_TO_NDVI, train_diffusion_superres
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation
    for mod in (train_diffusion_superres, train_diffusion_SAR_TO_NDVI, train_diffusion_generation, Aggregation_Sampling):
        p = mod.build_arg_parser()
        a = p.parse_args([])
        assert a.sampling_steps is None and a.eta == 0.0, mod.__name__
        a = p.parse_args(["--sampling_steps", "50", "--eta", "0.5"])
        assert a.sampling_steps == 50 and a.eta == 0.5, mod.__name__
