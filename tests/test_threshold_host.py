"""Dynamic x0 thresholding without a GPU: the command-line flag, `check_threshold`, the constructor
argument of the three `Diffusion` classes, what a default and a clip-only call do not call, the rank arithmetic, the float64
oracle's own identities, and every argument error of the new entry points."""
import ctypes as C
import math

import pytest
import torch

import prediction_oracle as PO
import threshold_oracle as TO
from oracle import diffusion_oracle as D
from test_prediction_host import _command_lines, _CountingLib, _stub, _train

LINES = ["superres", "sar", "generation", "evaluate", "evaluate_sar", "tiler"]


# ---------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("line", LINES)
def test_threshold_flag(line):
    from diffusionremotesensing_amd.cli import cli_prediction, cli_threshold
    parse = _command_lines()[line]
    assert cli_threshold(parse([])) == {"x0_threshold": None}
    args = parse(["--x0_clip", "0,1", "--x0_threshold", "0.995"])
    assert cli_threshold(args) == {"x0_threshold": 0.995}
    assert cli_prediction(args) == {"prediction": "eps", "x0_clip": (0.0, 1.0)}  # still the two-key dict
    assert cli_threshold(parse(["--x0_clip=-1,1", "--x0_threshold", "1"])) == {"x0_threshold": 1.0}
    for bad in ("0", "-0.5", "1.5", "nan", "p", ""):
        with pytest.raises(SystemExit):
            parse(["--x0_clip", "0,1", "--x0_threshold", bad])


@pytest.mark.parametrize("line", LINES)
def test_threshold_flag_in_the_help_texts(line, capsys):
    """Registered on every line; hidden on the trainers', whose help texts are recorded, shown on evaluate's and the tiler's."""
    with pytest.raises(SystemExit):
        _command_lines()[line](["--help"])
    shown = "--x0_threshold" in capsys.readouterr().out
    assert shown == (line in ("evaluate", "evaluate_sar", "tiler"))


def test_the_reference_flag_sets_do_not_carry_the_flag():
    import argparse

    from diffusionremotesensing_amd import cli, evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for p in (sr.build_arg_parser(), sar.build_arg_parser(), sar.train_arg_parser(), gen.build_arg_parser(),
              evaluate.evaluate_arg_parser(), cli.add_train_args(argparse.ArgumentParser())):
        assert "--x0_threshold" not in p._option_string_actions
    assert cli.cli_threshold(argparse.Namespace()) == {"x0_threshold": None}


def test_a_threshold_without_a_clip_ends_the_constructor(tmp_path):
    from diffusionremotesensing_amd.cli import cli_prediction, cli_threshold
    args = _command_lines()["evaluate"](["--x0_threshold", "0.9"])
    with pytest.raises(ValueError, match="needs x0_clip"):
        _stub(tmp_path, **cli_prediction(args), **cli_threshold(args))


# ---------------------------------------------------------------------------------------------
# check_threshold, Diffusion(x0_threshold=)
# ---------------------------------------------------------------------------------------------
def test_check_threshold():
    from diffusionremotesensing_amd.sampling import check_prediction, check_threshold
    assert check_threshold() is None and check_threshold(None, None) is None and check_threshold(None, (0.0, 1.0)) is None
    got = check_threshold(1, (0.0, 1.0))
    assert got == 1.0 and type(got) is float
    assert check_threshold(0.995, (-1.0, 1.0)) == 0.995 and check_threshold(1e-9, (0.0, 1.0)) == 1e-9
    for bad in (0, 0.0, -0.1, 1.0000001, 2, math.nan, math.inf, "0.5", (0.5,), True):
        with pytest.raises(ValueError, match="x0_threshold"):
            check_threshold(bad, (0.0, 1.0))
    with pytest.raises(ValueError, match="needs x0_clip"):
        check_threshold(0.5, None)
    assert check_prediction("v", (0, 1)) == ("v", (0.0, 1.0))  # two values, as ever


def test_constructor_argument_of_the_three_classes(tmp_path):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for cls in (None, sar.Diffusion, gen.Diffusion):
        assert _stub(tmp_path, cls).x0_threshold is None
        assert _stub(tmp_path, cls, x0_clip=(0, 1)).x0_threshold is None
        d = _stub(tmp_path, cls, prediction="v", x0_clip=(0, 1), x0_threshold=0.995)
        assert (d.prediction, d.x0_clip, d.x0_threshold) == ("v", (0.0, 1.0), 0.995)
        for bad in ({"x0_threshold": 0.5}, {"x0_clip": (0, 1), "x0_threshold": 0.0}, {"x0_clip": (0, 1), "x0_threshold": 1.5},
                    {"x0_clip": (0, 1), "x0_threshold": "0.5"}):
            with pytest.raises(ValueError, match="x0_threshold"):
                _stub(tmp_path, cls, **bad)


def test_the_threshold_is_not_written_into_snapshots(tmp_path):
    d = _stub(tmp_path, prediction="v", x0_clip=(0, 1), x0_threshold=0.9)
    d._save_snapshot(1, d.model)
    assert set(torch.load(tmp_path / "snapshot.pt")) == {"MODEL_STATE", "EPOCHS_RUN", "PREDICTION"}
    assert _stub(tmp_path, prediction="v").x0_threshold is None  # it loads as a network without one


def test_default_and_clip_only_calls_call_neither_new_symbol(tmp_path, monkeypatch):
    """A default run's chain set-up and an `x0_clip`-only `pred_to_eps_` reach the library through the old symbols only; a bad
    threshold on the schedule is caught before the first device call."""
    from diffusionremotesensing_amd import _lib, hip_ops, sampling
    counting = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counting)
    d = _train(_stub(tmp_path))

    def chain():
        return sampling.sample_chain(d, None, (1, 3, 8, 8), lambda *a: None, table_rows=1, sampling_steps=3,
                                     noise_source=lambda i, shape: torch.zeros(shape))
    for attrs, error in (({}, RuntimeError), ({"x0_clip": (0.0, 1.0)}, RuntimeError), ({"x0_threshold": 0.5}, ValueError),
                         ({"x0_clip": (0.0, 1.0), "x0_threshold": 2.0}, ValueError)):
        for k, v in attrs.items():
            setattr(d, k, v)
        with pytest.raises(error):
            chain()
        d.x0_clip, d.x0_threshold = None, None
    del d.x0_threshold  # a schedule without the attribute (the stubs of other tests)
    with pytest.raises(RuntimeError):
        chain()
    x, t = torch.zeros(2, 3, 4, 4), torch.ones(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU path: the clip-only call stops at its tensor checks
        hip_ops.pred_to_eps_(x, x, t, torch.ones(10), "v", (0.0, 1.0))
    new = ("drs_x0_quantile", "drs_pred_to_eps_dyn", "drs_x0_threshold_workspace_bytes")
    assert all(counting.calls[name] == 0 for name in new), counting.calls


def test_wrappers_check_their_arguments_before_any_tensor():
    from diffusionremotesensing_amd import hip_ops
    x, t, ah = torch.zeros(2, 3, 4, 4), torch.ones(2, dtype=torch.int64), torch.ones(10)
    with pytest.raises(ValueError, match="needs x0_clip"):
        hip_ops.pred_to_eps_(x, x, t, ah, "v", x0_threshold=0.5)
    for bad in (0.0, 1.5, -1.0, math.nan):
        with pytest.raises(ValueError, match="x0_threshold"):
            hip_ops.pred_to_eps_(x, x, t, ah, "v", (0.0, 1.0), x0_threshold=bad)
    with pytest.raises(RuntimeError, match="ROCm"):  # no CPU path
        hip_ops.pred_to_eps_(x, x, t, ah, "v", (0.0, 1.0), x0_threshold=0.5)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.x0_abs_quantile(x, x, t, ah, "v", (0.0, 1.0), 0.5)
    with pytest.raises(ValueError, match="prediction"):
        hip_ops.x0_abs_quantile(x, x, t, ah, "score", (0.0, 1.0), 0.5)


# ---------------------------------------------------------------------------------------------
# the rank, the oracle
# ---------------------------------------------------------------------------------------------
def test_rank_arithmetic():
    from diffusionremotesensing_amd.hip_ops import threshold_rank
    assert threshold_rank(1.0, 1) == 0 and threshold_rank(0.5, 1) == 0 and threshold_rank(1e-9, 1) == 0
    assert threshold_rank(1.0, 4097) == 4096 and threshold_rank(1e-9, 4097) == 0 and threshold_rank(0.5, 4097) == 2048
    assert threshold_rank(0.995, 3 * 256 * 256) == math.floor(0.995 * (3 * 256 * 256 - 1)) == 195623
    assert threshold_rank(1.0, 16 * 256 * 256) == 16 * 256 * 256 - 1
    for chw in (2, 7, 960, 4097):
        for k in range(0, chw - 1, max(1, chw // 13)):  # p between k and k + 1 of chw - 1 selects k
            assert threshold_rank((k + 0.5) / (chw - 1), chw) == k == TO.rank_of((k + 0.5) / (chw - 1), chw)
    for bad in (0.0, -0.5, 1.0000001, math.nan):
        with pytest.raises(ValueError):
            threshold_rank(bad, 10)
    # the rank is torch.quantile's interpolation="lower"
    g = torch.Generator().manual_seed(1)
    v = torch.randn(960, generator=g).abs().double()
    for p in (1e-9, 0.3, 0.5, 0.995, 1.0):
        assert torch.sort(v).values[threshold_rank(p, 960)] == torch.quantile(v, p, interpolation="lower")


@pytest.mark.parametrize("clip", [(0.0, 1.0), (-1.0, 1.0)])
def test_oracle_identities(clip):
    """A scale inside the range is the static clip; beyond it the thresholded x0 lies in the range, keeps the order of the
    values and leaves those at the centre where they are; non-finite values rank last and stay."""
    _, ah, _ = D.schedule("cosine", 50)
    lo, hi = clip
    c, r = TO.centre_and_half_range(clip)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 2, 5, 7), generator=g).double()
    inside = c + r * (torch.rand((3, 2, 5, 7), generator=g).double() * 1.8 - 0.9)
    t = torch.tensor([5, 20, 40])
    eps, _, s = TO.to_eps("x0", inside, x, ah, t, clip, 1.0)
    assert (s <= r).all() and torch.equal(eps, PO.to_eps("x0", inside, x, ah, t, clip)[0])
    wide = c + 3 * r * torch.randn((3, 2, 5, 7), generator=g).double()
    q, s = TO.threshold_x0(wide, clip, 0.9)
    assert (s > r).all() and q.min() >= lo and q.max() <= hi
    order = wide.flatten(1).argsort(dim=1)
    assert (q.flatten(1).gather(1, order).diff(dim=1) >= 0).all()
    assert not torch.equal(q, wide.clamp(lo, hi))
    assert torch.equal(s, (wide - c).abs().flatten(1).sort(dim=1).values[:, TO.rank_of(0.9, 70)])
    planted = wide.clone()
    planted[0, 0, 0, :3] = torch.tensor([math.nan, math.inf, -math.inf], dtype=torch.float64)
    q2, s2 = TO.threshold_x0(planted, clip, 0.5)
    assert torch.isnan(q2[0, 0, 0, 0]) and q2[0, 0, 0, 1] == math.inf and q2[0, 0, 0, 2] == -math.inf
    assert torch.isfinite(s2).all() and torch.isfinite(q2[1:]).all()
    _, s3 = TO.threshold_x0(planted, clip, 1.0)  # the maximum of image 0 is +inf: the static clip
    q3, _ = TO.threshold_x0(planted, clip, 1.0)
    assert s3[0] == math.inf and torch.equal(q3[0].flatten()[3:], planted[0].flatten()[3:].clamp(lo, hi))


# ---------------------------------------------------------------------------------------------
# the entry points: argument checks, no launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["drs_x0_quantile", "drs_pred_to_eps_dyn"])
def test_entry_points_refuse_bad_arguments_without_a_gpu(name):
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, name)
    what = name[4:].encode()
    bufs = [(C.c_float * 8)() for _ in range(7)]  # host memory: every call fails its checks, or has nothing to do, before a launch
    pred, x, t, ah, out, scale, ws = (C.cast(b, C.c_void_p) for b in bufs)
    big = 1 << 20

    def call(pred=pred, pu=None, w=0.0, x=x, t=t, ah=ah, T=10, kind=1, lo=0.0, hi=1.0, k=0, out=out, scale=scale, n=1, chw=4,
             ws=ws, nbytes=big):
        return fn(pred, pu, w, x, t, ah, T, kind, lo, hi, k, out, scale, n, chw, ws, nbytes, None)

    def refused(status, word, **kw):
        assert call(**kw) == status, kw
        msg = lib.drs_last_error()
        assert what in msg and word in msg, (kw, msg)
    for missing in ("pred", "x", "t", "ah", "out", "ws"):
        refused(1, b"null pointer", **{missing: None})
    if name == "drs_x0_quantile":
        refused(1, b"null pointer", scale=None)
    refused(1, b"kind", kind=3)
    refused(1, b"kind", kind=-1)
    refused(1, b"lo < hi", lo=1.0, hi=1.0)
    refused(1, b"lo < hi", lo=1.0, hi=0.0)
    refused(1, b"lo < hi", lo=math.nan)
    refused(1, b"cfg_scale", pu=pred, w=math.inf)
    refused(1, b"cfg_scale", pu=pred, w=math.nan)
    refused(2, b"chw", n=-1)
    refused(2, b"chw", chw=-1)
    refused(2, b"chw", chw=1 << 32)
    refused(2, b"noise_steps", T=0)
    refused(1, b"one buffer", x=out)
    refused(1, b"rank", k=-1)
    refused(1, b"rank", k=4)
    need = lib.drs_x0_threshold_workspace_bytes(1)
    refused(1, b"workspace", nbytes=need - 1)
    refused(1, b"workspace", nbytes=0)
    # nothing to do: DRS_OK before the rank, the workspace size or anything on the device is looked at
    assert call(n=0, k=99, nbytes=0) == 0 and call(chw=0, k=0, nbytes=0) == 0


def test_workspace_size_grows_with_the_batch():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    one = lib.drs_x0_threshold_workspace_bytes(1)
    assert lib.drs_x0_threshold_workspace_bytes(0) == 0 and lib.drs_x0_threshold_workspace_bytes(-3) == 0
    assert one >= (2048 + 1024 + 1024) * 4 and lib.drs_x0_threshold_workspace_bytes(16) == 16 * one
    assert lib.drs_abi_version() == 8  # new symbols, nothing changed
