"""DPM-Solver++(2M) sampling without a GPU: the logSNR level list, the float64 oracle (against the DDIM oracle and on an analytic
Gaussian problem), the `sampling_plan` that carries the solver, the argument checks of Diffusion.sample, drs_dpm_step and
drs_blend_step_dpm, the driver's choice between first and second order, and the CLI flags."""
import ctypes as C

import pytest
import torch

import ddim_oracle as O
import dpm_oracle as P
from oracle import diffusion_oracle as D

SCHEDULES = [("linear", 50), ("linear", 1000), ("cosine", 1500)]


# ---------------------------------------------------------------------------------------------
# levels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", SCHEDULES)
def test_logsnr_timesteps(kind, T):
    from diffusionremotesensing_amd.sampling import logsnr_timesteps
    _, ah, _ = D.schedule(kind, T)
    for S in (1, 2, 10, T - 1):
        ts = logsnr_timesteps(ah, S)
        assert len(ts) == S and all(type(t) is int for t in ts)
        assert all(a > b for a, b in zip(ts, ts[1:]))  # strictly descending, hence distinct
        assert 1 <= ts[-1] and ts[0] <= T - 1
        assert ts == P.logsnr_levels(ah, S)
    assert logsnr_timesteps(ah, 1) == [T - 1]
    assert logsnr_timesteps(ah, 2) == [T - 1, 1]
    assert logsnr_timesteps(ah, T - 1) == list(range(T - 1, 0, -1))
    for S in (0, -1, T):
        with pytest.raises(ValueError):
            logsnr_timesteps(ah, S)


def test_logsnr_timesteps_are_uniform_in_logsnr_where_the_table_allows():
    """T = 1000, S = 10: no level had to be pushed, every one is the nearest to its target, so consecutive logSNR steps differ
    by less than the table's own resolution around them allows - far from the factor 4 to 6 of the uniform-in-t levels."""
    from diffusionremotesensing_amd.sampling import ddim_timesteps, logsnr_timesteps
    _, ah, _ = D.schedule("linear", 1000)

    def ratios(ts):
        lam = [P.lam(ah, t) for t in ts]
        h = [b - a for a, b in zip(lam, lam[1:])]
        return max(h) / min(h)
    assert ratios(logsnr_timesteps(ah, 10)) < 1.3
    assert ratios(ddim_timesteps(1000, 10)) > 4


def test_chain_moves_takes_the_spacing_and_is_unchanged_without_it():
    from diffusionremotesensing_amd.sampling import Move, chain_moves, ddim_timesteps, logsnr_timesteps
    assert chain_moves(50, 7) == [Move(a, b) for a, b in zip([49, 41, 33, 25, 17, 9, 1], [41, 33, 25, 17, 9, 1, 0])]
    assert chain_moves(5) == [Move(4, 3), Move(3, 2), Move(2, 1), Move(1, 0)]
    assert chain_moves(50, 7, spacing="uniform") == chain_moves(50, 7)
    for resample, jump in ((1, 1), (3, 2)):
        lv = ddim_timesteps(30, 6) + [0]
        from diffusionremotesensing_amd.sampling import inpaint_schedule
        assert chain_moves(30, 6, resample, jump) == [Move(lv[p], lv[q]) for p, q in inpaint_schedule(6, resample, jump)]
    _, ah, _ = D.schedule("cosine", 50)
    lv = logsnr_timesteps(ah, 10) + [0]
    assert chain_moves(50, 10, spacing="logsnr", alpha_hat=ah) == [Move(a, b) for a, b in zip(lv, lv[1:])]
    with pytest.raises(ValueError):
        chain_moves(50, 10, spacing="logsnr")  # no table


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", [("linear", 1000), ("cosine", 1500)])
def test_oracle_first_order_move_is_the_ddim_eta0_move(kind, T):
    _, ah, _ = D.schedule(kind, T)
    g = torch.Generator().manual_seed(5)
    x, e = (torch.randn((2, 3, 4, 4), generator=g, dtype=torch.float64) for _ in range(2))
    for t, tp in ((T - 1, T - 31), (T - 1, 1), (500, 499), (7, 1), (1, 0), (T - 1, 0), (40, 0)):
        got, x0 = P.step(x, e, None, None, t, tp, ah)
        want = O.step(x, e, None, t, tp, 0.0, ah)
        assert ((got - want).abs().max() / want.abs().max()).item() <= 1e-12, (kind, t, tp)
        at = float(ah[t])
        assert torch.allclose(x0, (x - (1 - at) ** 0.5 * e) / at ** 0.5, rtol=1e-13, atol=0)
    if kind == "cosine":  # alpha_hat[0] = 1: the move to level 0 lands on the x0 prediction
        got, x0 = P.step(x, e, None, None, T - 1, 0, ah)
        assert torch.equal(got, x0)


@pytest.mark.parametrize("kind,T", [("linear", 1000), ("cosine", 1500)])
@pytest.mark.parametrize("S", [10, 20])
def test_oracle_2m_halves_the_ddim_error_on_the_gaussian_problem(kind, T, S):
    """Data N(0, 0.25): eps(x, t) = x s_t / (0.25 ah_t + 1 - ah_t) and the exact end point is x_T sqrt(var_0 / var_L0).  On the
    logSNR levels the 2M chain ends with at most half the DDIM chain's relative error (float64; measured: 7.4x and 8.5x lower
    on linear T = 1000 at S = 10 / 20, 10.9x and 6.9x on cosine T = 1500)."""
    _, ah, _ = D.schedule(kind, T)
    e2, e1 = P.gauss_chain_error(ah, S, "dpmpp_2m"), P.gauss_chain_error(ah, S, "ddim")
    print(f"gaussian anchor [{kind} T={T} S={S}]: DDIM {e1:.3e}  2M {e2:.3e}  ratio {e1 / e2:.2f}")
    assert e2 <= 0.5 * e1, (kind, S, e1, e2)


# ---------------------------------------------------------------------------------------------
# argument checks (no engine, no GPU)
# ---------------------------------------------------------------------------------------------
def test_sampling_plan_and_its_checks():
    from diffusionremotesensing_amd.sampling import (SamplingSteps, check_sampling_args, check_solver_known, plan_of,
                                                     sampling_plan)
    plan = sampling_plan(10, solver="dpmpp_2m")
    assert isinstance(plan, int) and plan == 10 and int(plan) == 10 and plan.solver == "dpmpp_2m" and plan.spacing is None
    assert plan_of(None) == plan_of(10) == plan_of(sampling_plan(10)) == ("ddim", "uniform")
    assert plan_of(plan) == ("dpmpp_2m", "logsnr") and plan_of(sampling_plan(10, "dpmpp_2m", "uniform")) == ("dpmpp_2m", "uniform")
    assert plan_of(sampling_plan(10, spacing="logsnr")) == ("ddim", "logsnr")
    assert "dpmpp_2m" in repr(plan) and type(plan + 1) is int
    for args in ((None, "dpmpp_2m"), (None, "ddim", "logsnr"), (10, "euler"), (10, "ddim", "karras"), (2.5, "dpmpp_2m"),
                 (True, "dpmpp_2m")):
        with pytest.raises(ValueError):
            sampling_plan(*args)
    check_sampling_args(50, plan, 0.0)
    check_sampling_args(50, sampling_plan(10, spacing="logsnr"), 0.5)
    check_sampling_args(50, None, 0.0)
    for S, eta in ((plan, 0.5), (sampling_plan(50, "dpmpp_2m"), 0.0), (sampling_plan(0, "dpmpp_2m"), 0.0)):
        with pytest.raises(ValueError):
            check_sampling_args(50, S, eta)
    known = torch.zeros(1)
    check_solver_known(plan, None, None)
    check_solver_known(sampling_plan(10, spacing="logsnr"), known, known)
    check_solver_known(None, known, known)
    with pytest.raises(ValueError, match="known"):
        check_solver_known(plan, known, known)
    assert SamplingSteps(7) == 7 and plan_of(SamplingSteps(7, "dpmpp_2m")) == ("dpmpp_2m", "logsnr")
    for args in ((7, "euler"), (7, "ddim", "karras"), (2.5,), (True,)):  # built directly: the same checks as sampling_plan
        with pytest.raises(ValueError):
            SamplingSteps(*args)


def test_evaluate_summary_names_solver_and_spacing():
    from diffusionremotesensing_amd.evaluate import sampling_line
    from diffusionremotesensing_amd.sampling import sampling_plan
    assert sampling_line(20, 0.0) == sampling_line(sampling_plan(20), 0.0) == "DDIM 20 steps eta 0.0"  # as it was
    assert sampling_line(sampling_plan(20, spacing="logsnr"), 0.5) == "DDIM 20 steps eta 0.5, logsnr-spaced levels"
    assert sampling_line(sampling_plan(20, "dpmpp_2m"), 0.0) == "DPM-Solver++(2M) 20 steps eta 0.0, logsnr-spaced levels"
    assert sampling_line(sampling_plan(20, "dpmpp_2m", "uniform"), 0.0) == "DPM-Solver++(2M) 20 steps eta 0.0, uniform-spaced levels"


def test_diffusion_sample_rejects_bad_solver_requests():
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as GenDiffusion
    from diffusionremotesensing_amd.sampling import sampling_plan
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
    tiler = split_aggregation_sampling(torch.zeros(1, 3, 8, 8), 8, 8, 2, d, "cpu")
    known = {"known": torch.zeros(3, 16, 16), "known_mask": torch.zeros(16, 16)}
    calls = [lambda **kw: d.sample(1, m, torch.zeros(3, 8, 8), **kw),
             lambda **kw: ds.sample(1, m, torch.zeros(2, 16, 16), **kw),
             lambda **kw: dg.sample(1, m, target_class=torch.tensor([1]), **kw),
             lambda **kw: d.sample_ensemble(2, m, torch.zeros(3, 8, 8), **kw),
             lambda **kw: d.evaluate(m, [(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 16, 16))], **kw),
             lambda **kw: tiler.aggregation_sampling(aggregation="final", **kw),
             lambda **kw: tiler.aggregation_sampling(aggregation="per_step", **kw)]
    two_m = sampling_plan(5, solver="dpmpp_2m")
    for call in calls:
        for kw in ({"sampling_steps": two_m, "eta": 0.5}, {"sampling_steps": sampling_plan(T, solver="dpmpp_2m")}):
            with pytest.raises(ValueError):
                call(**kw)
        for kw in ({"sampling_steps": two_m}, {"sampling_steps": sampling_plan(5, spacing="logsnr")},
                   {"sampling_steps": sampling_plan(5, "dpmpp_2m", "uniform")}):
            with pytest.raises(AssertionError, match="engine"):  # valid arguments get as far as the engine
                call(**kw)
    # known pixels: refused with the multistep solver, taken by DDIM on either spacing
    for dd, cond in ((d, (torch.zeros(3, 8, 8),)), (dg, ())):
        with pytest.raises(ValueError, match="known"):
            dd.sample_known(1, m, *cond, **known, sampling_steps=two_m)
        with pytest.raises(ValueError, match="known"):
            dd.sample_ensemble(2, m, *cond, **known, sampling_steps=two_m)
        with pytest.raises(AssertionError, match="engine"):
            dd.sample_known(1, m, *cond, **known, sampling_steps=sampling_plan(5, spacing="logsnr"))
    with pytest.raises(ValueError, match="known"):
        ds.sample_known(1, m, torch.zeros(2, 16, 16), torch.zeros(1, 16, 16), torch.zeros(16, 16), sampling_steps=two_m)


def _host_buffer():
    buf = (C.c_float * 64)()  # host memory: every call below must fail validation before any launch
    return buf, C.cast(buf, C.c_void_p)


def test_dpm_step_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf, p = _host_buffer()

    def call(x=p, ec=p, eu=None, w=0.0, hist=p, tq=20, t=10, tp=5, ah=p, T=50, n=16):
        return lib.drs_dpm_step(x, ec, eu, w, hist, tq, t, tp, ah, T, n, None)

    for kw, msg in (({"x": None}, b"null pointer"), ({"ec": None}, b"null pointer"), ({"hist": None}, b"null pointer"),
                    ({"ah": None}, b"null pointer"), ({"tp": 10}, b"t_p"), ({"tp": 11}, b"t_p"), ({"tp": -1}, b"t_p"),
                    ({"t": 50, "tq": -1}, b"t_p"), ({"tq": 10}, b"t_q"), ({"tq": 9}, b"t_q"), ({"tq": 50}, b"t_q"),
                    ({"tq": -2}, b"t_q"), ({"tq": 20, "tp": 0}, b"level 0"), ({"n": -1}, b"numel")):
        assert call(**kw) == 1, kw  # DRS_ERR_ARG
        assert msg in lib.drs_last_error(), (kw, lib.drs_last_error())
    assert call(n=0) == 0 and call(n=0, tq=-1, tp=0) == 0  # valid moves of nothing: no launch


def test_blend_step_dpm_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf, p = _host_buffer()

    def call(scene=p, eps=p, org=p, w=p, hist=p, unc=None, n=1, Cc=1, S=2, Hs=2, Ws=2, tq=20, t=10, tp=5, ah=p, T=50):
        return lib.drs_blend_step_dpm(scene, eps, org, w, hist, unc, n, Cc, S, Hs, Ws, tq, t, tp, ah, T, None)

    for kw, msg in (({"scene": None}, b"null"), ({"eps": None}, b"null"), ({"org": None}, b"null"), ({"w": None}, b"null"),
                    ({"hist": None}, b"null"), ({"ah": None}, b"null"), ({"tp": 10}, b"t_p"), ({"tp": -1}, b"t_p"),
                    ({"t": 50, "tq": -1}, b"t_p"), ({"tq": 10}, b"t_q"), ({"tq": 50}, b"t_q"), ({"tq": -2}, b"t_q"),
                    ({"tq": 20, "tp": 0}, b"level 0")):
        assert call(**kw) == 1, kw  # DRS_ERR_ARG
        assert msg in lib.drs_last_error(), (kw, lib.drs_last_error())
    assert call(S=3) == 2 and call(n=0) == 2  # DRS_ERR_SHAPE, as drs_blend_step


def test_dpm_wrappers_have_no_cpu_fallback():
    from diffusionremotesensing_amd import hip_ops
    x = torch.zeros(4)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.dpm_step_(x, x, torch.zeros(4), None, 10, 5, torch.ones(50))
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.reverse_step_(x, x, None, 10, 5, alpha=None, alpha_hat=torch.ones(50), beta=None, ddim=True,
                              hist=torch.zeros(4), t_q=-1)


# ---------------------------------------------------------------------------------------------
# the driver: which moves are second order
# ---------------------------------------------------------------------------------------------
class _Schedule:
    def __init__(self, kind, T):
        self.noise_steps, self.device = T, "cpu"
        self.alpha, self.alpha_hat, self.beta = D.schedule(kind, T)


class _Engine:
    """check_faults raises a range fault at its `fail_at`-th call (0: never)."""
    def __init__(self, fail_at=0):
        self.calls, self.fail_at = 0, fail_at

    def check_faults(self):
        self.calls += 1
        if self.calls == self.fail_at:
            from diffusionremotesensing_amd import _lib
            raise _lib.RangeFault("drs_unet_check_faults failed with status 6: test")


def _drive(monkeypatch, engine, S=8, every=None, spacing=None):
    """`sample_chain` on the CPU with an `update` hook that records (t, t_to, t_q) and keeps the history's protocol."""
    from diffusionremotesensing_amd import hip_ops, sampling
    monkeypatch.setattr(hip_ops, "timestep_table", lambda T, n, device: torch.arange(T).unsqueeze(1).expand(T, n))
    if every is not None:
        monkeypatch.setattr(sampling.run_reverse_chain, "__defaults__", (None, every, None))
    sch = _Schedule("cosine", 50)
    seen = []

    def update(x, eps, noise, t, t_to, hist=None, t_q=-1):
        assert noise is None and hist is not None and hist.shape == x.shape
        seen.append((t, t_to, t_q))
        hist.fill_(float(t))
        x.add_(1.0)
    src_calls = []

    def src(i, shape):
        src_calls.append(i)
        return torch.zeros(shape)
    x = sampling.sample_chain(sch, engine, (1, 1, 2, 2), lambda e, x, t, first: torch.zeros_like(x), table_rows=1,
                              noise_source=src, sampling_steps=sampling.sampling_plan(S, "dpmpp_2m", spacing), update=update)
    return sch, seen, src_calls, x


def test_sample_chain_orders_of_the_2m_moves(monkeypatch):
    from diffusionremotesensing_amd.sampling import ddim_timesteps, logsnr_timesteps
    sch, seen, src_calls, x = _drive(monkeypatch, _Engine())
    lv = logsnr_timesteps(sch.alpha_hat, 8)
    assert [s[0] for s in seen] == lv and [s[1] for s in seen] == lv[1:] + [0]
    # first move: no history; last move (to level 0): first order; every other one second order on the level before
    assert [s[2] for s in seen] == [-1] + lv[:-2] + [-1]
    assert src_calls == [50] and x.flatten()[0].item() == 8.0  # x_T and nothing else is drawn
    _, seen, _, _ = _drive(monkeypatch, _Engine(), spacing="uniform")
    assert [s[0] for s in seen] == ddim_timesteps(50, 8)
    _, seen, _, _ = _drive(monkeypatch, _Engine(), S=1)
    assert seen == [(49, 0, -1)]


def test_sample_chain_resumes_first_order_after_a_roll_back(monkeypatch):
    """The checkpoint holds x, not the history: the move a roll-back resumes at finds the x0 of a later move there and is taken
    first order; the one after it is second order again."""
    from diffusionremotesensing_amd.sampling import logsnr_timesteps
    sch, seen, _, x = _drive(monkeypatch, _Engine(fail_at=2), every=3)
    lv = logsnr_timesteps(sch.alpha_hat, 8)
    assert [s[0] for s in seen] == lv[:6] + lv[3:]  # moves 3..5 run again
    assert seen[6] == (lv[3], lv[4], -1) and seen[7] == (lv[4], lv[5], lv[3])
    assert x.flatten()[0].item() == 8.0


def test_existing_update_hooks_are_called_as_before(monkeypatch):
    """A DDIM or ancestral chain hands its `update` hook five positional arguments and nothing else."""
    from diffusionremotesensing_amd import hip_ops, sampling
    monkeypatch.setattr(hip_ops, "timestep_table", lambda T, n, device: torch.arange(T).unsqueeze(1).expand(T, n))
    sch = _Schedule("cosine", 20)
    for S, spacing in ((None, None), (5, None), (5, "logsnr")):
        seen = []

        def update(*args, **kw):
            assert len(args) == 5 and not kw
            seen.append(args[3:])
        sampling.sample_chain(sch, _Engine(), (1, 1, 2, 2), lambda e, x, t, first: torch.zeros_like(x), table_rows=1,
                              noise_source=lambda i, shape: torch.zeros(shape), update=update,
                              sampling_steps=sampling.sampling_plan(S, spacing=spacing) if spacing else S)
        lv = sampling.chain_levels(20, S, spacing or "uniform", sch.alpha_hat) + [0]
        assert seen == [(a, b if S else None) for a, b in zip(lv, lv[1:])]


# ---------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------
def test_solver_flags_on_the_tiler_and_evaluate_parsers():
    """--solver / --spacing next to --sampling_steps; the three trainers' parsers keep the flag set they had."""
    from diffusionremotesensing_amd import Aggregation_Sampling, evaluate, train_diffusion_superres
    from diffusionremotesensing_amd.sampling import plan_of
    from diffusionremotesensing_amd.train_diffusion_superres import cli_sampling_steps
    from diffusionremotesensing_amd.train_diffusion_superres import add_solver_args
    for p in (Aggregation_Sampling.build_arg_parser(), add_solver_args(evaluate.evaluate_arg_parser("superres")),
              add_solver_args(evaluate.evaluate_arg_parser("sar_to_ndvi"))):  # (as evaluate.main builds its parser)
        a = p.parse_args(["--sampling_steps", "20"])
        assert a.solver == "ddim" and a.spacing is None and type(cli_sampling_steps(a)) is int
        assert cli_sampling_steps(p.parse_args([])) is None
        plan = cli_sampling_steps(p.parse_args(["--sampling_steps", "20", "--solver", "dpmpp_2m"]))
        assert plan == 20 and plan_of(plan) == ("dpmpp_2m", "logsnr")
        plan = cli_sampling_steps(p.parse_args(["--sampling_steps", "20", "--spacing", "logsnr"]))
        assert plan == 20 and plan_of(plan) == ("ddim", "logsnr")
        with pytest.raises(SystemExit):
            p.parse_args(["--solver", "heun"])
        with pytest.raises(ValueError):
            cli_sampling_steps(p.parse_args(["--solver", "dpmpp_2m"]))  # no --sampling_steps
    assert cli_sampling_steps(train_diffusion_superres.build_arg_parser().parse_args(["--sampling_steps", "7"])) == 7
