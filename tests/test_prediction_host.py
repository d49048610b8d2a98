"""v- and x0-prediction without a GPU: the float64 oracle's identities, the Min-SNR weights of the three
parameterisations, the command-line flags, what a default run does not call, the wiring of `Diffusion(prediction=, x0_clip=)`
into the objective and the snapshot, and the argument checks of the two entry points."""
import collections
import math

import pytest
import torch

import prediction_oracle as PO
from oracle import diffusion_oracle as D

SCHEDULES = (("cosine", 1500), ("linear", 1000))


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", SCHEDULES)
@pytest.mark.parametrize("pred", ["v", "x0"])
def test_oracle_round_trips(kind, T, pred):
    _, ah, _ = D.schedule(kind, T)
    g = torch.Generator().manual_seed(3)
    x0, eps = torch.rand((2, 3, 4, 5), generator=g).double(), torch.randn((2, 3, 4, 5), generator=g).double()
    for t in (1, T // 2, T - 1):
        a, s = PO.a_s(ah, t)
        x_t = a * x0 + s * eps
        p = PO.from_eps(pred, eps, x_t, ah, t)
        back, _ = PO.to_eps(pred, p, x_t, ah, t)
        scale = float((x_t / s).abs().max() + 1)  # (the x0 form divides by s: its terms are that large)
        assert (back - eps).abs().max().item() <= 1e-12 * scale, (t, pred)
        assert (PO.to_x0(pred, p, x_t, ah, t) - x0).abs().max().item() <= 1e-12 * float(1 / a), (t, pred)
        # x_t = a x0 + s eps recovered from (v, x_t): x0 = a x_t - s v, eps = s x_t + a v
        v = PO.from_eps("v", eps, x_t, ah, t)
        assert (a * (a * x_t - s * v) + s * (s * x_t + a * v) - x_t).abs().max().item() <= 1e-12 * float(x_t.abs().max())
        # a clip that does not bite changes nothing
        wide, _ = PO.to_eps(pred, p, x_t, ah, t, clip=(-1e9, 1e9))
        assert (wide - eps).abs().max().item() <= 1e-12 * scale


def test_oracle_clip_keeps_non_finite_values_and_bounds_x0():
    _, ah, _ = D.schedule("cosine", 50)
    x = torch.zeros((1, 1, 1, 4), dtype=torch.float64)
    p = torch.tensor([2.0, -3.0, math.inf, math.nan], dtype=torch.float64).view(1, 1, 1, 4)
    eps, _ = PO.to_eps("x0", p, x, ah, 10, clip=(0.0, 1.0))
    a, s = PO.a_s(ah, 10)
    assert eps[0, 0, 0, 0].item() == pytest.approx(float(-a / s)) and eps[0, 0, 0, 1].item() == 0.0
    assert not torch.isfinite(eps[0, 0, 0, 2:]).any()


# ---------------------------------------------------------------------------------------------
# Min-SNR weights
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,T", SCHEDULES)
@pytest.mark.parametrize("gamma", [1.0, 5.0])
def test_min_snr_weights_of_the_three_predictions(kind, T, gamma):
    from diffusionremotesensing_amd.losses import min_snr_weights
    _, ah, _ = D.schedule(kind, T)
    w = {p: min_snr_weights(ah, gamma, p) for p in PO.KINDS}
    for p in PO.KINDS:
        assert w[p].dtype == torch.float32 and w[p].shape == ah.shape and not torch.isnan(w[p]).any(), p
        want = PO.weights(p, ah, gamma)
        assert torch.equal(w[p], want.float()) or (w[p].double() - want).abs().max() <= 1e-7 * float(want.abs().max()), p
    # today's table, bit for bit, with and without the new argument
    a = ah.double()
    today = torch.clamp(float(gamma) / (a / (1.0 - a)), max=1.0).float()
    assert torch.equal(w["eps"], today) and torch.equal(min_snr_weights(ah, gamma), today)
    # one weighting of the x0 error: w_v (SNR + 1) == w_x0 == w_eps SNR where SNR is finite
    snr = a / (1.0 - a)
    fin = torch.isfinite(snr)
    wx0 = w["x0"].double()[fin]
    assert (w["v"].double()[fin] * (snr[fin] + 1) - wx0).abs().max() <= 1e-6 * gamma
    assert (w["eps"].double()[fin] * snr[fin] - wx0).abs().max() <= 1e-6 * gamma


def test_min_snr_weights_where_alpha_hat_is_one():
    from diffusionremotesensing_amd.losses import min_snr_weights
    ah = torch.tensor([1.0, 0.5, 0.0])
    assert min_snr_weights(ah, 5.0, "eps").tolist() == [0.0, 1.0, 1.0]
    assert min_snr_weights(ah, 5.0, "v").tolist() == [0.0, 0.5, 0.0]
    assert min_snr_weights(ah, 5.0, "x0").tolist() == [5.0, 1.0, 0.0]
    with pytest.raises(ValueError, match="prediction"):
        min_snr_weights(ah, 5.0, "score")


# ---------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------
def _command_lines():
    from diffusionremotesensing_amd import Aggregation_Sampling, evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    need = ["--image_size", "32", "--model_name", "m", "--loss", "MSE"]
    return {"superres": lambda argv: sr.parse_train_args(need + ["--magnification_factor", "2"] + argv),
            "sar": lambda argv: sar.train_main_parser().parse_args(need + argv),
            "generation": lambda argv: gen.train_main_parser().parse_args(need + argv),
            "evaluate": lambda argv: evaluate.cli_arg_parser("superres").parse_args(argv),
            "evaluate_sar": lambda argv: evaluate.cli_arg_parser("sar_to_ndvi").parse_args(argv),
            "tiler": lambda argv: Aggregation_Sampling.build_arg_parser().parse_args(argv)}


@pytest.mark.parametrize("line", ["superres", "sar", "generation", "evaluate", "evaluate_sar", "tiler"])
def test_prediction_flags(line):
    from diffusionremotesensing_amd.cli import cli_prediction
    parse = _command_lines()[line]
    assert cli_prediction(parse([])) == {"prediction": "eps", "x0_clip": None}
    assert cli_prediction(parse(["--prediction", "v", "--x0_clip", "0,1"])) == {"prediction": "v", "x0_clip": (0.0, 1.0)}
    assert cli_prediction(parse(["--prediction", "x0", "--x0_clip=-1,1"])) == {"prediction": "x0", "x0_clip": (-1.0, 1.0)}
    assert cli_prediction(parse(["--x0_clip", "none"])) == {"prediction": "eps", "x0_clip": None}
    for bad in (["--prediction", "score"], ["--x0_clip", "1"], ["--x0_clip", "1,0"], ["--x0_clip", "a,b"], ["--x0_clip", "0,1,2"]):
        with pytest.raises(SystemExit):
            parse(bad)


def test_the_reference_flag_sets_carry_neither_flag():
    import argparse

    from diffusionremotesensing_amd import cli, evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for p in (sr.build_arg_parser(), sar.build_arg_parser(), sar.train_arg_parser(), gen.build_arg_parser(),
              evaluate.evaluate_arg_parser(), cli.add_train_args(argparse.ArgumentParser())):
        assert not {"--prediction", "--x0_clip"} & set(p._option_string_actions)
    assert cli.cli_prediction(argparse.Namespace()) == {"prediction": "eps", "x0_clip": None}


# ---------------------------------------------------------------------------------------------
# Diffusion(prediction=, x0_clip=)
# ---------------------------------------------------------------------------------------------
class _CountingLib:
    """The loaded library with every call through the ctypes binding counted by name (as tests/test_loss_host.py)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def _stub(tmp_path, cls=None, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    extra = {"magnification_factor": 2, "Degradation_type": "DownBlur"} if cls is None else {}
    return (cls or Diffusion)("cosine", torch.nn.Linear(3, 2), str(tmp_path / "snapshot.pt"), noise_steps=10, device="cpu",
                              image_size=8, **extra, **kw)


def _train(d, loss="MSE", **kw):
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=[], val_loader=None, patience=5, loss=loss, verbose=False, **kw)
    return d


def test_constructor_arguments_of_the_three_classes(tmp_path):
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for cls in (None, sar.Diffusion, gen.Diffusion):
        d = _stub(tmp_path, cls)
        assert (d.prediction, d.x0_clip) == ("eps", None)
        d = _stub(tmp_path, cls, prediction="v", x0_clip=(0, 1))
        assert (d.prediction, d.x0_clip) == ("v", (0.0, 1.0))
        for bad in ({"prediction": "score"}, {"prediction": None}, {"x0_clip": (1.0, 1.0)}, {"x0_clip": (1.0, 0.0)},
                    {"x0_clip": 1.0}, {"x0_clip": (0.0, 1.0, 2.0)}, {"x0_clip": ("a", "b")}):
            with pytest.raises(ValueError):
                _stub(tmp_path, cls, **bad)


def test_default_run_and_chain_set_up_call_neither_new_symbol(tmp_path, monkeypatch):
    from diffusionremotesensing_amd import _lib, sampling
    counting = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "_lib", counting)
    d = _train(_stub(tmp_path))
    assert type(d.train_state.loss_function) is torch.nn.MSELoss
    # a default chain: the set-up runs up to the first device call, which has no CPU path; a bad attribute is caught before it
    for attrs, error in (({}, RuntimeError), ({"x0_clip": (1.0, 0.0)}, ValueError), ({"prediction": "score"}, ValueError)):
        for k, v in attrs.items():
            setattr(d, k, v)
        with pytest.raises(error):
            sampling.sample_chain(d, None, (1, 3, 8, 8), lambda *a: None, table_rows=1, sampling_steps=3,
                                  noise_source=lambda i, shape: torch.zeros(shape))
        d.prediction, d.x0_clip = "eps", None
    assert counting.calls["drs_noise_v_target"] == 0 and counting.calls["drs_pred_to_eps"] == 0


def test_default_train_step_goes_through_noise_images_and_predict(tmp_path, monkeypatch):
    """The two methods existing tests replace are what a default step and an x0 step call; a v step forms x_t and v in one
    launch instead of `noise_images`."""
    seen = []
    d = _stub(tmp_path)
    monkeypatch.setattr(d, "noise_images", lambda x, t: (seen.append("noise_images"), (x + 1, x + 2))[1])
    x0 = torch.zeros(2, 3, 8, 8)
    x_t, target = d._noised_target(x0, torch.ones(2, dtype=torch.int64))
    assert torch.equal(x_t, x0 + 1) and torch.equal(target, x0 + 2) and seen == ["noise_images"]
    d.prediction = "x0"
    x_t, target = d._noised_target(x0, torch.ones(2, dtype=torch.int64))
    assert torch.equal(x_t, x0 + 1) and target is x0 and seen == ["noise_images"] * 2
    d.prediction = "v"
    with pytest.raises(RuntimeError, match="ROCm"):  # no eager fallback
        d._noised_target(x0, torch.ones(2, dtype=torch.int64))
    assert seen == ["noise_images"] * 2


@pytest.mark.parametrize("prediction", ["v", "x0"])
def test_prediction_wires_its_table_into_the_loss(tmp_path, prediction):
    from diffusionremotesensing_amd.losses import DiffusionLoss, min_snr_weights
    d = _train(_stub(tmp_path, prediction=prediction), loss_weighting="min_snr", min_snr_gamma=2.0)
    fn = d.train_state.loss_function
    assert type(fn) is DiffusionLoss and torch.equal(fn.table, min_snr_weights(d.alpha_hat, 2.0, prediction))
    assert torch.equal(d.train_state.objective.val.table, fn.table)
    assert not torch.equal(fn.table, min_snr_weights(d.alpha_hat, 2.0))


@pytest.mark.parametrize("prediction", ["v", "x0"])
def test_perceptual_loss_needs_an_eps_network(tmp_path, prediction):
    with pytest.raises(ValueError, match="Perceptual_noise"):
        _train(_stub(tmp_path, prediction=prediction), loss="MSE+Perceptual_noise")


def test_snapshot_records_the_prediction(tmp_path, capsys):
    for name, prediction in (("e", "eps"), ("v", "v"), ("x", "x0")):
        (tmp_path / name).mkdir()
        d = _stub(tmp_path / name, prediction=prediction)
        d._save_snapshot(3, d.model)
        saved = torch.load(tmp_path / name / "snapshot.pt")
        if prediction == "eps":
            assert set(saved) == {"MODEL_STATE", "EPOCHS_RUN"}  # the reference's file
        else:
            assert set(saved) == {"MODEL_STATE", "EPOCHS_RUN", "PREDICTION"} and saved["PREDICTION"] == prediction
        assert _stub(tmp_path / name, prediction=prediction).epochs_run == 3
    for name, other in (("e", "v"), ("v", "eps"), ("v", "x0"), ("x", "eps")):
        with pytest.raises(ValueError, match="predicts"):
            _stub(tmp_path / name, prediction=other)


# ---------------------------------------------------------------------------------------------
# the entry points: argument checks, no launch
# ---------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes as C

    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    assert lib.drs_noise_v_target(None, None, None, None, 10, None, None, 1, 1, None) == 1
    assert b"noise_v_target" in lib.drs_last_error() and b"null pointer" in lib.drs_last_error()
    assert lib.drs_pred_to_eps(None, None, 0.0, None, None, None, 10, 0, 0, 0.0, 0.0, None, 1, 1, None) == 1
    assert b"pred_to_eps" in lib.drs_last_error() and b"null pointer" in lib.drs_last_error()
    buf = (C.c_float * 8)()  # host memory: every call below fails its checks, or has nothing to do, before any launch
    p = C.cast(buf, C.c_void_p)
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 10, 3, 0, 0.0, 0.0, p, 1, 1, None) == 1 and b"kind" in lib.drs_last_error()
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 10, 1, 1, 1.0, 1.0, p, 1, 1, None) == 1 and b"lo < hi" in lib.drs_last_error()
    assert lib.drs_pred_to_eps(p, p, math.inf, p, p, p, 10, 1, 0, 0.0, 0.0, p, 1, 1, None) == 1
    assert b"cfg_scale" in lib.drs_last_error()
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 10, 1, 0, 0.0, 0.0, p, -1, 1, None) == 2
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 0, 1, 0, 0.0, 0.0, p, 1, 1, None) == 2
    assert lib.drs_noise_v_target(p, p, p, p, 10, p, p, 1, -1, None) == 2
    assert lib.drs_noise_v_target(p, p, p, p, 10, p, p, 1, 1, None) == 1 and b"one buffer" in lib.drs_last_error()
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 10, 1, 0, 0.0, 0.0, p, 0, 4, None) == 0
    assert lib.drs_pred_to_eps(p, None, 0.0, p, p, p, 10, 1, 0, 0.0, 0.0, p, 4, 0, None) == 0
    assert lib.drs_abi_version() == 8


def test_wrappers_have_no_cpu_path():
    from diffusionremotesensing_amd import hip_ops
    x = torch.zeros(2, 3, 4, 4)
    t = torch.ones(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.noise_v_target(x, x, t, torch.ones(10))
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.pred_to_eps_(x, x, t, torch.ones(10), "v")
    with pytest.raises(ValueError, match="prediction"):
        hip_ops.pred_to_eps_(x, x, t, torch.ones(10), "score")
