"""LR-consistent sampling without a GPU: the un-rounded DownBlur operator against the uint8 pipeline it
describes, the projector's properties in float64, the refusals, the command-line flags, where `sample_chain` projects, and
the argument checks of the new entry points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import consistency_oracle as CO
from oracle import degradation_oracle as DO
from oracle import diffusion_oracle as D
from test_prediction_host import _command_lines, _stub

# |A_y X A_x^T - the uint8 pipeline| on `smooth_scene`: the largest value measured over CASES is 2.48 LSB (S = 64, m = 2,
# radius 0.5: eight rounding passes of half an LSB each and the resize's clip); the bar is twice that.
MEASURED_LSB = 2.48
CASES = [(S, m, r) for S, m in ((24, 2), (64, 2), (20, 4)) for r in (0.0, 0.5, 1.0)]


def smooth_scene(S, bands=3):
    y, x = np.mgrid[0:S, 0:S] / S
    img = [0.5 + 0.25 * np.sin(2 * np.pi * (1.0 + 0.5 * c) * x + 0.3 * c) * np.cos(2 * np.pi * (0.75 + 0.25 * c) * y) + 0.15 * (x - y)
           for c in range(bands)]
    return np.clip(np.round(np.stack(img) * 255), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,m,radius", CASES)
def test_operator_vs_the_uint8_pipeline(S, m, radius):
    from diffusionremotesensing_amd.consistency import SeparableOperator
    hr = smooth_scene(S)
    lr, _ = DO.downblur(hr, S // m, S // m, radius)
    op = SeparableOperator.downblur((S, S), m, radius)
    assert op.hr_shape == (S, S) and op.lr_shape == (S // m, S // m)
    diff = np.abs(op.apply(hr.astype(np.float64) / 255.0) - lr.astype(np.float64)).max() * 255.0
    print(f"S={S} m={m} radius={radius}: {diff:.3f} LSB")
    assert diff <= 2 * MEASURED_LSB
    # the package's matrices are the oracle's, which restates them on its own
    A_y, A_x = CO.downblur_matrices(S, S, m, radius)
    assert np.abs(A_y - op.A_y).max() < 1e-14 and np.abs(A_x - op.A_x).max() < 1e-14
    assert np.allclose(op.A_y.sum(axis=1), 1.0, atol=1e-14)  # a constant image stays what it is


def test_operator_shapes_and_constructors():
    from diffusionremotesensing_amd.consistency import SeparableOperator
    op = SeparableOperator.downblur((20, 28), 4, 0.5)  # the reference's swapped size: (W // m, H // m)
    assert op.A_y.shape == (7, 20) and op.A_x.shape == (5, 28) and op.lr_shape == (7, 5)
    op = SeparableOperator.downblur((20, 28), 4, 0.5, lr_hw=(5, 7))  # the tiler's scene
    assert op.lr_shape == (5, 7)
    box = SeparableOperator.box((6, 8), 2)
    x = np.arange(48.0).reshape(6, 8)
    assert np.array_equal(box.apply(x), x.reshape(3, 2, 4, 2).mean(axis=(1, 3)))
    same = SeparableOperator.from_matrices(box.A_y, box.A_x)
    assert np.array_equal(same.A_y, box.A_y) and same.hr_shape == (6, 8)
    for bad in (lambda: SeparableOperator.downblur((3, 3), 4, 0.5), lambda: SeparableOperator.downblur((8, 8), 2, "random"),
                lambda: SeparableOperator.downblur((8, 8), 2, -1.0), lambda: SeparableOperator.box((6, 8), 4),
                lambda: SeparableOperator(np.zeros(3), np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------
# the projector, float64
# ---------------------------------------------------------------------------------------------
def _project64(op, x, y, damping, strength=1.0):
    f = op.factors(damping)
    yt = f["P_y"].T @ y @ f["P_x"]
    return x + strength * f["U_y"] @ (f["G"] * (yt - f["D_y"] @ x @ f["D_x"].T)) @ f["U_x"].T


@pytest.mark.parametrize("radius", [0.0, 0.5])
def test_undamped_projection_is_exact_and_idempotent(radius):
    from diffusionremotesensing_amd.consistency import SeparableOperator
    rng = np.random.default_rng(3)
    op = SeparableOperator.downblur((24, 24), 2, radius)
    x, y = rng.random((24, 24)), rng.random((12, 12))
    p = _project64(op, x, y, 0.0)
    assert np.abs(op.apply(p) - y).max() < 1e-12
    assert np.abs(_project64(op, p, y, 0.0) - p).max() < 1e-12
    assert np.array_equal(_project64(op, x, y, 0.0, strength=0.0), x)
    want, _ = CO.Projection(op.A_y, op.A_x, 0.0).project(x, y)  # the oracle's own SVD
    assert np.abs(want - p).max() < 1e-12


def test_residual_grows_with_the_damping():
    from diffusionremotesensing_amd.consistency import SeparableOperator
    rng = np.random.default_rng(4)
    for radius in (0.5, 1.0):
        op = SeparableOperator.downblur((24, 24), 2, radius)
        x, y = rng.random((24, 24)), rng.random((12, 12))
        res = [np.sqrt(np.mean((op.apply(_project64(op, x, y, d)) - y) ** 2)) for d in (1e-4, 1e-3, 1e-2, 1e-1, 1.0)]
        assert all(a < b for a, b in zip(res, res[1:])), res
        assert res[-1] < np.sqrt(np.mean((op.apply(x) - y) ** 2))  # and any damping still reduces it


def test_an_ill_conditioned_operator_needs_damping():
    from diffusionremotesensing_amd.consistency import LRConsistency, SeparableOperator
    op = SeparableOperator.downblur((64, 64), 2, 1.5)
    with pytest.raises(ValueError, match="damping"):
        op.factors(0.0)
    with pytest.raises(ValueError, match="damping"):
        op.projector(0.0, "cpu")
    f = op.factors(0.01)
    assert np.isfinite(f["G"]).all() and f["G"].max() <= 50.0 + 1e-9  # s / (s^2 + d^2) <= 1 / (2 d)
    assert SeparableOperator.downblur((64, 64), 2, 1.0).factors(0.0)["G"].max() < 1e4
    for bad in (-0.1, math.nan, math.inf, "0.1", True):
        with pytest.raises(ValueError, match="damping"):
            op.factors(bad)
        with pytest.raises(ValueError, match="damping"):
            LRConsistency(damping=bad)


def test_projector_tensors():
    from diffusionremotesensing_amd.consistency import SeparableOperator
    op = SeparableOperator.downblur((20, 28), 4, 0.5)
    p = op.projector(0.01, "cpu")
    assert [tuple(t.shape) for t in (p.D_y, p.D_x, p.U_y, p.U_x, p.G, p.Pt_y, p.Pt_x)] == \
        [(7, 20), (5, 28), (20, 7), (28, 5), (7, 5), (7, 7), (5, 5)]
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (p.D_y, p.D_x, p.U_y, p.U_x, p.G))
    f = op.factors(0.01)
    assert np.allclose(f["P_y"] @ f["D_y"], op.A_y, atol=1e-14) and np.allclose(f["D_y"] @ f["U_y"], np.diag(f["s_y"]), atol=1e-14)
    with pytest.raises(ValueError, match="observation"):
        p.prepare(torch.zeros(1, 3, 5, 7))


# ---------------------------------------------------------------------------------------------
# the request and its refusals
# ---------------------------------------------------------------------------------------------
def test_request_values():
    from diffusionremotesensing_amd.consistency import LRConsistency, SeparableOperator, check_lr_consistency
    r = LRConsistency()
    assert (r.blur_radius, r.damping, r.strength, r.operator) == (None, 0.01, 1.0, None)
    assert check_lr_consistency(None) is None and check_lr_consistency(r) is r
    for bad in ({"blur_radius": "random"}, {"blur_radius": -1}, {"strength": math.nan}, {"strength": "1"}, {"operator": np.eye(2)}):
        with pytest.raises(ValueError):
            LRConsistency(**bad)
    with pytest.raises(ValueError, match="LRConsistency"):
        check_lr_consistency(True)
    op = SeparableOperator.box((8, 8), 2)
    assert LRConsistency(operator=op).operator_for(None, (8, 8)) is op
    with pytest.raises(ValueError, match="takes"):
        LRConsistency(operator=op).operator_for(None, (16, 16))


def test_the_diffusion_attribute(tmp_path):
    from diffusionremotesensing_amd.consistency import LRConsistency
    d = _stub(tmp_path)
    assert d.lr_consistency is None and d.blur_radius == 0.5
    req = LRConsistency()
    assert req.radius_for(d) == 0.5 and LRConsistency(blur_radius=1.0).radius_for(d) == 1.0
    assert req.operator_for(d, (8, 8)).lr_shape == (4, 4)
    d.blur_radius = "random"  # drawn per dataset object by the trainer: the request must name the number
    with pytest.raises(ValueError, match="blur_radius"):
        req.operator_for(d, (8, 8))
    assert LRConsistency(blur_radius=0.7).operator_for(d, (8, 8)).lr_shape == (4, 4)
    d.lr_consistency = req
    d._save_snapshot(1, d.model)
    assert set(torch.load(tmp_path / "snapshot.pt")) == {"MODEL_STATE", "EPOCHS_RUN"}  # not in snapshots


def test_bsrgan_is_refused(tmp_path):
    from diffusionremotesensing_amd.consistency import LRConsistency, SeparableOperator
    d = _stub(tmp_path)
    d.Degradation_type, d.lr_consistency = "BSRGAN", LRConsistency()
    lr = torch.zeros(3, 4, 4)
    with pytest.raises(ValueError, match="DownBlur"):
        d.sample(1, d.model, lr, sampling_steps=3, noise_source=lambda i, shape: torch.zeros(shape))
    with pytest.raises(ValueError, match="DownBlur"):
        d.evaluate(d.model, [], lr_consistency=LRConsistency())
    d.Degradation_type = "DownBlurNoise"
    assert LRConsistency().operator_for(d, (8, 8)).lr_shape == (4, 4)
    d.Degradation_type = "BSRGAN"  # an explicit operator stands for whatever made the LR image
    assert LRConsistency(operator=SeparableOperator.box((8, 8), 2)).operator_for(d, (8, 8)).lr_shape == (4, 4)


def test_the_other_samplers_refuse_the_attribute(tmp_path):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd.consistency import LRConsistency
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    src = {"noise_source": lambda i, shape: torch.zeros(shape), "sampling_steps": 3}
    d = _stub(tmp_path, sar.Diffusion)
    d.lr_consistency = LRConsistency()
    with pytest.raises(ValueError, match="super-resolution"):
        d.sample(1, d.model, torch.zeros(1, 2, 8, 8), **src)
    g = _stub(tmp_path, gen.Diffusion)
    g.lr_consistency = LRConsistency()
    with pytest.raises(ValueError, match="super-resolution"):
        g.sample(1, g.model, target_class=None, **src)
    d.lr_consistency = "on"
    with pytest.raises(ValueError, match="LRConsistency"):
        d.sample(1, d.model, torch.zeros(1, 2, 8, 8), **src)


def test_the_update_hook_is_refused(tmp_path):
    from diffusionremotesensing_amd import sampling
    from diffusionremotesensing_amd.consistency import LRConsistency
    d = _stub(tmp_path)
    d.lr_consistency = LRConsistency()
    with pytest.raises(ValueError, match="update hook"):
        sampling.sample_chain(d, None, (1, 3, 8, 8), lambda *a: None, table_rows=1, sampling_steps=3,
                              noise_source=lambda i, shape: torch.zeros(shape), update=lambda *a, **k: None,
                              lr_img=torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="update hook"):
        d._sample_chain(d.model, (1, 3, 8, 8), lambda *a: None, table_rows=1, generate_video=False, noise_source=None,
                        sampling_steps=3, eta=0.0, update=lambda *a, **k: None, lr_img=torch.zeros(1, 3, 4, 4))
    with pytest.raises(ValueError, match="ensemble"):
        d.evaluate(d.model, [], lr_consistency=LRConsistency(), ensemble=4)


# ---------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------
FLAGS = ("--lr_consistency", "--lr_damping", "--lr_strength", "--lr_blur_radius")


@pytest.mark.parametrize("line", ["evaluate", "tiler"])
def test_consistency_flags(line):
    from diffusionremotesensing_amd.cli import cli_consistency
    from diffusionremotesensing_amd.consistency import LRConsistency
    parse = _command_lines()[line]
    assert cli_consistency(parse([])) == {"lr_consistency": None}
    req = cli_consistency(parse(["--lr_consistency"]))["lr_consistency"]
    assert isinstance(req, LRConsistency) and (req.blur_radius, req.damping, req.strength) == (None, 0.01, 1.0)
    req = cli_consistency(parse(["--lr_consistency", "--lr_damping", "0", "--lr_strength", "0.5", "--lr_blur_radius", "1.0"]))
    req = req["lr_consistency"]
    assert (req.blur_radius, req.damping, req.strength) == (1.0, 0.0, 0.5)
    assert cli_consistency(parse(["--lr_consistency", "false"])) == {"lr_consistency": None}
    for flag, value in (("--lr_damping", "0.1"), ("--lr_strength", "0.5"), ("--lr_blur_radius", "1")):
        with pytest.raises(ValueError, match="belong to --lr_consistency"):
            cli_consistency(parse([flag, value]))
    for bad in (["--lr_damping", "-1"], ["--lr_damping", "nan"], ["--lr_damping", "d"], ["--lr_strength", "inf"],
                ["--lr_strength", ""], ["--lr_blur_radius", "random"], ["--lr_blur_radius", "-0.5"]):
        with pytest.raises(SystemExit):
            parse(["--lr_consistency"] + bad)


@pytest.mark.parametrize("line", ["superres", "sar", "generation", "evaluate", "evaluate_sar", "tiler"])
def test_consistency_flags_in_the_help_texts(line, capsys):
    """Shown by evaluate (superres) and the tiler; the trainers and the SAR -> NDVI evaluation do not have them at all."""
    parse = _command_lines()[line]
    with pytest.raises(SystemExit):
        parse(["--help"])
    out = capsys.readouterr().out
    for flag in FLAGS:
        assert (flag in out) == (line in ("evaluate", "tiler")), (line, flag)
    if line not in ("evaluate", "tiler"):
        with pytest.raises(SystemExit):
            parse(["--lr_consistency"])


def test_the_reference_flag_sets_do_not_carry_the_flags():
    import argparse

    from diffusionremotesensing_amd import cli, evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for p in (sr.build_arg_parser(), sar.build_arg_parser(), sar.train_arg_parser(), gen.build_arg_parser(),
              evaluate.evaluate_arg_parser(), cli.add_train_args(argparse.ArgumentParser()),
              cli.add_prediction_args(argparse.ArgumentParser())):
        assert not set(FLAGS) & set(p._option_string_actions)
    assert cli.cli_consistency(argparse.Namespace()) == {"lr_consistency": None}


def test_evaluate_table_rows():
    from diffusionremotesensing_amd.evaluate import format_table
    row = {"psnr": 30.0, "ssim": 0.9, "sam": 1.0, "ergas": 2.0}
    plain = format_table({"model": row, "bicubic": row})
    assert "LR RMSE" not in plain and "model_free" not in plain
    table = format_table({"model": {**row, "lr_rmse": 1e-4}, "model_free": {**row, "lr_rmse": 2e-2}, "bicubic": {**row, "lr_rmse": 1e-2}})
    lines = table.splitlines()
    assert "LR RMSE" in lines[0] and [ln.split()[0] for ln in lines[1:]] == ["model", "model_free", "bicubic"]
    assert "0.0001" in lines[1] and "0.02" in lines[2]


# ---------------------------------------------------------------------------------------------
# where the chain projects
# ---------------------------------------------------------------------------------------------
class _Schedule:
    Degradation_type, magnification_factor, blur_radius = "DownBlur", 2, 0.5

    def __init__(self, T, **attrs):
        self.noise_steps, self.device = T, "cpu"
        self.alpha, self.alpha_hat, self.beta = D.schedule("cosine", T)
        for k, v in attrs.items():
            setattr(self, k, v)


class _Engine:
    def check_faults(self):
        pass


class _FakeOps:
    """`hip_ops` as `sample_chain` and `LRProjector.prepare` see it, every call recorded as (name, level or None)."""

    def __init__(self):
        self.calls = []

    def timestep_table(self, T, n, device):
        return torch.arange(T).unsqueeze(1).expand(T, n)

    def sep_apply(self, y, d_y, d_x):
        self.calls.append(("sep_apply", None))
        return torch.einsum("ij,bcjk,lk->bcil", d_y, y, d_x)

    def pred_to_eps_(self, pred, x, t, alpha_hat, prediction="eps", x0_clip=None, **kw):
        self.calls.append(("pred_to_eps_", int(t[0])))
        return pred

    def lr_consistent_eps_(self, eps, x, t, alpha_hat, yt, projector, strength=1.0):
        assert tuple(yt.shape) == (2, 3, 4, 4) and tuple(projector.G.shape) == (4, 4) and t.numel() == 2
        self.calls.append(("lr_consistent_eps_", int(t[0]), strength))
        return eps

    def reverse_step_(self, x, eps, noise, t, t_to, **kw):
        self.calls.append(("reverse_step_", t))

    def terminal_step_(self, x, pred, noise, t, t_to, *a, **kw):
        self.calls.append(("terminal_step_", t))


def _drive(monkeypatch, sch, sampling_steps, **kw):
    from diffusionremotesensing_amd import consistency, sampling
    ops = _FakeOps()
    monkeypatch.setattr(sampling, "hip_ops", ops)
    monkeypatch.setattr(consistency, "hip_ops", ops)
    draws = []

    def src(i, shape):
        draws.append(i)
        return torch.zeros(shape)
    sampling.sample_chain(sch, _Engine(), (2, 3, 8, 8), lambda e, x, t, first: torch.zeros_like(x), table_rows=2,
                          noise_source=src, sampling_steps=sampling_steps, lr_img=torch.zeros(1, 3, 4, 4), **kw)
    return ops.calls, draws


@pytest.mark.parametrize("S", [None, 4], ids=["ancestral", "ddim"])
def test_one_projection_per_reverse_move(monkeypatch, S):
    from diffusionremotesensing_amd.consistency import LRConsistency
    from diffusionremotesensing_amd.sampling import chain_levels
    sch = _Schedule(8, lr_consistency=LRConsistency(strength=0.75))
    calls, draws = _drive(monkeypatch, sch, S)
    levels = chain_levels(8, S)
    assert calls[0] == ("sep_apply", None) and sum(c[0] == "sep_apply" for c in calls) == 1  # the observation, once per chain
    want = []
    for t in levels:  # conversion (forced on), projection, update - in this order, at every level
        want += [("pred_to_eps_", t), ("lr_consistent_eps_", t, 0.75), ("reverse_step_", t)]
    assert calls[1:] == want
    assert draws == ([8] + levels[:-1] if S is None else [8])  # the draws of the plain chain


def test_no_projection_without_the_attribute(monkeypatch):
    calls, _ = _drive(monkeypatch, _Schedule(8), 4)
    assert [c[0] for c in calls] == ["reverse_step_"] * 4  # what a default chain launches today
    calls, _ = _drive(monkeypatch, _Schedule(8, lr_consistency=None, x0_clip=(0.0, 1.0)), 4)
    assert [c[0] for c in calls] == ["pred_to_eps_", "reverse_step_"] * 4


def test_no_projection_at_the_terminal_level(monkeypatch):
    from diffusionremotesensing_amd.consistency import LRConsistency
    from diffusionremotesensing_amd.sampling import chain_levels, rescale_zero_terminal_snr
    sch = _Schedule(8, lr_consistency=LRConsistency(), prediction="v", zero_terminal_snr=True)
    sch.alpha_hat = rescale_zero_terminal_snr(sch.alpha_hat)
    calls, _ = _drive(monkeypatch, sch, 4)
    levels = chain_levels(8, 4)
    assert levels[0] == 7
    assert calls[1] == ("terminal_step_", 7)
    assert [c for c in calls if c[0] == "lr_consistent_eps_"] == [("lr_consistent_eps_", t, 1.0) for t in levels[1:]]


def test_known_pixels_and_the_solver_keep_their_moves(monkeypatch):
    """`sample_known` and `dpmpp_2m` need nothing of their own: the projection sits in front of whatever takes the move."""
    from diffusionremotesensing_amd.consistency import LRConsistency
    from diffusionremotesensing_amd.sampling import sampling_plan
    sch = _Schedule(8, lr_consistency=LRConsistency())
    calls, _ = _drive(monkeypatch, sch, sampling_plan(3, "dpmpp_2m"))
    assert [c[0] for c in calls[1:]] == ["pred_to_eps_", "lr_consistent_eps_", "reverse_step_"] * 3
    calls, draws = _drive(monkeypatch, sch, 3, known=torch.zeros(3, 8, 8), known_mask=torch.ones(8, 8, dtype=torch.bool))
    assert [c[0] for c in calls[1:]] == ["pred_to_eps_", "lr_consistent_eps_", "reverse_step_"] * 3 and len(draws) == 3


# ---------------------------------------------------------------------------------------------
# the entry points: argument checks, no launch
# ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    bufs = [(C.c_float * 64)() for _ in range(12)]  # host memory: every call fails a check before it launches
    x, eps, t, ah, yt, dy, dx, uy, ux, g, out, ws = (C.cast(b, C.c_void_p) for b in bufs)
    shape = dict(n=1, c=1, H=4, W=4, h=2, w=2)
    big = 1 << 20

    def apply(x=x, dy=dy, dx=dx, out=out, ws=ws, nbytes=big, **s):
        s = {**shape, **s}
        return lib.drs_sep_apply(x, dy, dx, out, s["n"], s["c"], s["H"], s["W"], s["h"], s["w"], ws, nbytes, None)

    def project(x=x, yt=yt, dy=dy, dx=dx, uy=uy, ux=ux, g=g, strength=1.0, out=out, ws=ws, nbytes=big, **s):
        s = {**shape, **s}
        return lib.drs_sep_project(x, yt, dy, dx, uy, ux, g, strength, out, s["n"], s["c"], s["H"], s["W"], s["h"], s["w"], ws,
                                   nbytes, None)

    def project_eps(eps=eps, x=x, t=t, ah=ah, T=10, yt=yt, dy=dy, dx=dx, uy=uy, ux=ux, g=g, strength=1.0, ws=ws, nbytes=big, **s):
        s = {**shape, **s}
        return lib.drs_sep_project_eps(eps, x, t, ah, T, yt, dy, dx, uy, ux, g, strength, s["n"], s["c"], s["H"], s["W"], s["h"],
                                       s["w"], ws, nbytes, None)

    def refused(fn, what, status, word, **kw):
        assert fn(**kw) == status, (what, kw)
        msg = lib.drs_last_error()
        assert what in msg and word in msg, (kw, msg)
    need = lib.drs_sep_workspace_bytes(1, 1, 4, 4, 2, 2)
    assert need >= (max(2 * 4, 4 * 2) + 2 * 2) * 4
    for fn, what, pointers in ((apply, b"sep_apply", ("x", "dy", "dx", "out", "ws")),
                               (project, b"sep_project", ("x", "yt", "dy", "dx", "uy", "ux", "g", "out", "ws")),
                               (project_eps, b"sep_project_eps", ("eps", "x", "t", "ah", "yt", "dy", "dx", "uy", "ux", "g", "ws"))):
        for missing in pointers:
            refused(fn, what, 1, b"null pointer", **{missing: None})
        refused(fn, what, 2, b"bands", c=17)
        for extent in shape:
            refused(fn, what, 2, b">= 1", **{extent: 0})
            refused(fn, what, 2, b">= 1", **{extent: -3})
        refused(fn, what, 4, b"workspace", nbytes=need - 1)
        refused(fn, what, 4, b"workspace", nbytes=0)
    for fn, what in ((project, b"sep_project"), (project_eps, b"sep_project_eps")):
        for bad in (math.nan, math.inf, -math.inf):
            refused(fn, what, 1, b"strength", strength=bad)
    refused(project_eps, b"sep_project_eps", 1, b"noise_steps", T=0)
    refused(project_eps, b"sep_project_eps", 1, b"one buffer", x=eps)
    # strength 0 has nothing to do: eps keeps its bits and nothing is launched (host memory would fault)
    assert project_eps(strength=0.0) == 0 and project(strength=0.0, out=x) == 0


def test_workspace_size():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    assert lib.drs_sep_workspace_bytes(0, 3, 8, 8, 4, 4) == 0 and lib.drs_sep_workspace_bytes(1, 3, 8, 8, 4, -1) == 0
    one, two = lib.drs_sep_workspace_bytes(1, 3, 256, 256, 128, 128), lib.drs_sep_workspace_bytes(2, 3, 256, 256, 128, 128)
    assert one == 3 * (256 * 128 + 128 * 128) * 4 + 16 and two - 16 == 2 * (one - 16)
    assert lib.drs_abi_version() == 8  # new symbols, nothing changed


def test_wrappers_have_no_cpu_fallback():
    from diffusionremotesensing_amd import consistency, hip_ops
    op = consistency.SeparableOperator.downblur((8, 8), 2, 0.5)
    x, y = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm"):
        consistency.degrade(x, op)
    with pytest.raises(RuntimeError, match="ROCm"):
        consistency.project(x, y, op.projector(0.01, "cpu"))
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.lr_consistent_eps_(x, x.clone(), torch.ones(1, dtype=torch.int64), torch.ones(10), y, op.projector(0.01, "cpu"))
    with pytest.raises(ValueError, match="strength"):
        consistency.project(x, y, op.projector(0.01, "cpu"), strength=math.nan)
