"""Host side of fine-tuning with frozen BatchNorm (no device): `freeze_batchnorm`, `finetune.py`, the three trainers' flags,
`Diffusion.train(init_from=, freeze=, freeze_bn=)`, the train state, and the check that the GPU test's oracle can tell the two
BatchNorm regimes apart."""
import argparse
import os

import pytest
import torch
import torch.nn as nn


def _models():
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    return {"superres": lambda: Residual_Attention_UNet_superres(3, 3, "cpu"),
            "sar": lambda: Residual_Attention_UNet_SAR_TO_NDVI(2, 1, "cpu"),
            "generation": lambda: Residual_Attention_UNet_generation(3, 3, 10, "cpu")}


def _bn_modes(m):
    return {b.training for b in m.modules() if isinstance(b, nn.BatchNorm2d)}


@pytest.mark.parametrize("variant", ["superres", "sar", "generation"])
def test_freeze_batchnorm_is_sticky(variant):
    import copy
    m = _models()[variant]()
    assert m.training and _bn_modes(m) == {True}
    assert m.freeze_batchnorm() is m
    assert m.training and _bn_modes(m) == {False}
    others = {mod.training for mod in m.modules() if not isinstance(mod, nn.BatchNorm2d)}
    assert others == {True}
    m.train()  # what the trainers and `sample` call
    assert m.training and _bn_modes(m) == {False}
    m.eval()
    assert not m.training and _bn_modes(m) == {False}
    m.train()
    assert _bn_modes(m) == {False}
    c = copy.deepcopy(m).train()  # (the EMA copy)
    assert _bn_modes(c) == {False}
    m.freeze_batchnorm(False)
    assert m.training and _bn_modes(m) == {True}
    m.eval()
    assert _bn_modes(m) == {False}
    m.train()
    assert _bn_modes(m) == {True}
    m.eval().freeze_batchnorm(False)
    assert _bn_modes(m) == {False}  # an eval-mode model stays in eval mode
    # the state_dict knows nothing of it
    assert list(m.state_dict()) == list(_models()[variant]().state_dict())


def test_engine_reads_the_regime_from_the_modules():
    m = _models()["superres"]()
    eng = m.hip_engine()
    assert eng._frozen_bn(m) is False
    m.freeze_batchnorm()
    assert eng._frozen_bn(m) is True
    m.freeze_batchnorm(False)
    m.ups[1].batch_norm.eval()
    with pytest.raises(RuntimeError, match="1 of the model's 21 BatchNorm2d layers are in eval mode"):
        eng._frozen_bn(m)
    # the plain torch way: model.train() and every BatchNorm2d in .eval()
    m.train()
    for b in m.modules():
        if isinstance(b, nn.BatchNorm2d):
            b.eval()
    assert eng._frozen_bn(m) is True


def test_prefix_matching():
    from diffusionremotesensing_amd.finetune import freeze_parameters, frozen_names
    m = _models()["superres"]()
    names = [n for n, _ in m.named_parameters()]
    assert frozen_names(m, ()) == []
    got = frozen_names(m, ("downs.", "LR_encoder."))
    assert got == [n for n in names if n.startswith("downs.") or n.startswith("LR_encoder.")] and len(got) == 6 + 14
    assert frozen_names(m, ("conv_blocks.0.conv1.0.weight",)) == ["conv_blocks.0.conv1.0.weight"]
    for bad in (("down.",), ("downs.", "lr_encoder."), ("",), ("downs.3",)):
        with pytest.raises(ValueError, match="matches no parameter"):
            frozen_names(m, bad)
    assert all(p.requires_grad for p in m.parameters())  # a refused call froze nothing
    with pytest.raises(ValueError, match="matches no parameter"):
        freeze_parameters(m, ("downs.", "nothing."))
    assert all(p.requires_grad for p in m.parameters())
    (n_off, n_on), (e_off, e_on) = freeze_parameters(m, ("downs.", "LR_encoder."))
    assert (n_off, n_on) == (20, len(names) - 20)
    assert e_off + e_on == sum(p.numel() for p in m.parameters()) and e_off == sum(p.numel() for n, p in m.named_parameters() if n in got)
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == got
    with pytest.raises(ValueError, match="leaves no parameter to train"):
        freeze_parameters(nn.Linear(3, 2), ("weight", "bias"))


def _parsers():
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    return {"superres": sr.parse_train_args, "sar": lambda argv: sar.train_main_parser().parse_args(argv),
            "generation": lambda argv: gen.train_main_parser().parse_args(argv)}


@pytest.mark.parametrize("trainer", ["superres", "sar", "generation"])
def test_trainer_flags(trainer):
    from test_train_loop_host import _expected, _help_texts

    from diffusionremotesensing_amd.cli import cli_finetune
    parse = _parsers()[trainer]
    assert cli_finetune(parse([])) == {"freeze_bn": False, "freeze": (), "init_from": None}
    a = parse(["--freeze_bn", "--freeze", "downs.,conv_blocks.,LR_encoder.", "--init_from", "runs/s2/snapshot.pt"])
    assert cli_finetune(a) == {"freeze_bn": True, "freeze": ("downs.", "conv_blocks.", "LR_encoder."),
                               "init_from": "runs/s2/snapshot.pt"}
    assert cli_finetune(parse(["--freeze_bn", "False", "--freeze", "output."])) == {"freeze_bn": False, "freeze": ("output.",),
                                                                                     "init_from": None}
    for bad in (["--freeze", "downs.,,ups."], ["--freeze", ""], ["--init_from"]):
        with pytest.raises(SystemExit):
            parse(bad)
    assert cli_finetune(argparse.Namespace()) == {"freeze_bn": False, "freeze": (), "init_from": None}
    # accepted without a --help entry: the recorded help texts stand
    text = _help_texts()[trainer]
    assert text == _expected()["help"][trainer]
    assert not any("freeze" in line or "init_from" in line for line in text)


def test_launcher_passes_the_flags_to_train(monkeypatch):
    from diffusionremotesensing_amd import launcher
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    seen = {}

    class D:
        def __init__(self, **kw):
            pass

        def train(self, **kw):
            seen.update(kw)
    args = sar.train_main_parser().parse_args(["--freeze_bn", "--freeze", "ups.", "--init_from", "a.pt"])
    args.snapshot_folder_path = "."
    launcher.train_model(args, D, nn.Linear(2, 2), "cpu", [], None)
    assert (seen["freeze_bn"], seen["freeze"], seen["init_from"]) == (True, ("ups.",), "a.pt")


# ---- Diffusion.train(init_from=, freeze=, freeze_bn=) on a stub network ---------------------------------------------------
def _stub(tmp_path, model=None, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", model if model is not None else nn.Linear(3, 2), str(tmp_path / "run" / "snapshot.pt"),
                     noise_steps=10, device="cpu", magnification_factor=2, image_size=8, Degradation_type="DownBlur", **kw)


def _train(d, **kw):
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=[], val_loader=None, patience=5, loss="MSE", verbose=False, **kw)
    return d


def _snapshot(path, weight, epochs_run=37, **extra):
    src = nn.Linear(3, 2)
    with torch.no_grad():
        src.weight.fill_(weight)
        src.bias.fill_(weight)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({"MODEL_STATE": src.state_dict(), "EPOCHS_RUN": epochs_run, **extra}, path)
    return path


def test_init_from_rules(tmp_path, capsys):
    os.makedirs(tmp_path / "run")
    init = _snapshot(str(tmp_path / "pre" / "snapshot.pt"), 3.0)
    # no own snapshot: the other run's weights, epoch 0 (the empty loader still saves at epoch 0)
    d = _train(_stub(tmp_path), init_from=init)
    assert d.epochs_run == 0 and bool((d.model.weight == 3.0).all())
    assert "Starting from the weights of" in capsys.readouterr().out
    saved = torch.load(tmp_path / "run" / "snapshot.pt")
    assert saved["EPOCHS_RUN"] == 0 and bool((saved["MODEL_STATE"]["weight"] == 3.0).all())
    # the run's own snapshot wins
    _snapshot(str(tmp_path / "run" / "snapshot.pt"), 5.0, epochs_run=1)
    d = _train(_stub(tmp_path), init_from=init)
    assert d.epochs_run == 1 and bool((d.model.weight == 5.0).all())
    assert "Starting from the weights of" not in capsys.readouterr().out
    os.remove(tmp_path / "run" / "snapshot.pt")
    # the PREDICTION check applies
    v_init = _snapshot(str(tmp_path / "pre_v" / "snapshot.pt"), 4.0, PREDICTION="v")
    with pytest.raises(ValueError, match="predicts 'v'"):
        _train(_stub(tmp_path), init_from=v_init)
    with pytest.raises(ValueError, match="predicts 'eps'"):
        _train(_stub(tmp_path, prediction="v"), init_from=init)
    assert bool((_train(_stub(tmp_path, prediction="v"), init_from=v_init).model.weight == 4.0).all())
    os.remove(tmp_path / "run" / "snapshot.pt")
    # a shape mismatch names the key; missing / unknown keys are refused
    with pytest.raises(ValueError, match=r"weight has shape \(2, 3\), the model's is \(2, 5\)"):
        _train(_stub(tmp_path, model=nn.Linear(5, 2)), init_from=init)
    with pytest.raises(ValueError, match="keys differ"):
        _train(_stub(tmp_path, model=nn.Linear(3, 2, bias=False)), init_from=init)
    with pytest.raises(FileNotFoundError):
        _train(_stub(tmp_path), init_from=str(tmp_path / "nowhere.pt"))


def test_freeze_on_train(tmp_path, capsys):
    os.makedirs(tmp_path / "run")
    d = _train(_stub(tmp_path), freeze=("weight",))
    assert not d.model.weight.requires_grad and d.model.bias.requires_grad
    assert "Fine-tuning: 1 parameter tensors frozen (6 values), 1 trained (2 values); BatchNorm statistics updated" in capsys.readouterr().out
    assert (d.train_state.freeze_bn, d.train_state.freeze) == (False, ("weight",))
    with pytest.raises(ValueError, match="matches no parameter"):
        _train(_stub(tmp_path), freeze=("weights.",))
    with pytest.raises(ValueError, match="tuple of state_dict-key prefixes"):
        _train(_stub(tmp_path), freeze="weight")
    with pytest.raises(ValueError, match="freeze_bn needs one of the three UNet classes"):
        _train(_stub(tmp_path), freeze_bn=True)
    os.remove(tmp_path / "run" / "snapshot.pt")
    # a default run prints nothing new and freezes nothing
    d = _train(_stub(tmp_path))
    assert "Fine-tuning" not in capsys.readouterr().out and all(p.requires_grad for p in d.model.parameters())


def test_freeze_bn_on_train_with_a_unet(tmp_path, capsys):
    os.makedirs(tmp_path / "run")
    m = _models()["superres"]()
    d = _train(_stub(tmp_path, model=m), freeze_bn=True, freeze=("LR_encoder.",))
    assert m.training and _bn_modes(m) == {False}
    m.train()
    assert _bn_modes(m) == {False}
    assert "Fine-tuning: 14 parameter tensors frozen" in capsys.readouterr().out
    assert d.train_state.freeze_bn is True


def test_train_state_mismatch_raises(tmp_path):
    """train_state.pt carries freeze_bn / freeze; a resume that freezes something else is refused before anything is loaded."""
    os.makedirs(tmp_path / "run")
    _snapshot(str(tmp_path / "run" / "snapshot.pt"), 1.0, epochs_run=0)
    base = {"RAW_MODEL_STATE": None, "LR_SCHEDULE": None, "OPTIMIZER_STATE": None}
    path = str(tmp_path / "run" / "train_state.pt")
    torch.save({**base, "FREEZE_BN": False, "FREEZE": ("weight",)}, path)
    for kw in ({}, {"freeze": ("bias",)}, {"freeze": ("weight", "bias")}):
        if kw.get("freeze") == ("weight", "bias"):
            continue  # (refused earlier: nothing left to train)
        with pytest.raises(ValueError, match="--freeze weight: a resumed run must freeze the same"):
            _train(_stub(tmp_path), save_train_state=True, **kw)
    torch.save(dict(base), path)  # a file of a run that froze nothing
    with pytest.raises(ValueError, match=r"--freeze \(none\): a resumed run must freeze the same"):
        _train(_stub(tmp_path), save_train_state=True, freeze=("weight",))
    torch.save({**base, "FREEZE_BN": True, "FREEZE": ()}, path)
    with pytest.raises(ValueError, match="--freeze_bn True"):
        _train(_stub(tmp_path), save_train_state=True)


def test_train_state_records_the_freeze(tmp_path, monkeypatch):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    os.makedirs(tmp_path / "run")
    written = {}
    monkeypatch.setattr(torch.cuda, "get_rng_state", lambda device=None: torch.zeros(1, dtype=torch.uint8))
    monkeypatch.setattr(torch, "save", lambda obj, path: written.__setitem__(os.path.basename(str(path)), obj))
    _train(_stub(tmp_path), save_train_state=True, freeze=("weight",))
    assert (written["train_state.pt"]["FREEZE_BN"], written["train_state.pt"]["FREEZE"]) == (False, ("weight",))
    written.clear()
    _train(_stub(tmp_path), save_train_state=True)
    assert "FREEZE" not in written["train_state.pt"] and "FREEZE_BN" not in written["train_state.pt"]
    assert Diffusion.train.__defaults__[-3:] == (False, (), None)


# ---- the oracle can tell the regimes apart ---------------------------------------------------------------------------------
def test_batch_statistics_gradients_fail_the_frozen_bar(seeded_sd):
    """The float64 oracle's batch-statistics gradients on `tiny` against its frozen ones, at the bar the GPU test holds the
    frozen kernels to: far outside.  A kernel that still normalised with batch statistics could not pass test_gpu_frozen_bn."""
    from frozen_step import calibrated_sd, frozen_oracle_step
    from grad_check import MAX_REL_F32, REL_L2_F32, check_grads, grad_errors

    from diffusionremotesensing_amd import synthetic
    sd = calibrated_sd("superres", seeded_sd)
    # calibrated and perturbed: not the initial 0 / 1, not the plain calibration batch's either
    rm, rv = sd["bottle_neck.batch_norm1.running_mean"], sd["bottle_neck.batch_norm1.running_var"]
    assert rm.abs().max() > 0 and (rv - 1).abs().max() > 0 and bool((rv > 0).all())
    assert torch.equal(sd["conv_blocks.1.conv2.1.running_var"], sd["conv_blocks.1.batch_norm2.running_var"])
    assert calibrated_sd("superres", seeded_sd) is sd
    batch = (synthetic.tensor_normal("grads.tiny.x", (2, 3, 24, 40)), torch.tensor([1, 1499]),
             synthetic.tensor_uniform("grads.tiny.lr", (2, 3, 12, 20)), synthetic.tensor_normal("grads.tiny.noise", (2, 3, 24, 40)), 2)
    names = [n for n, _ in _models()["superres"]().named_parameters()]
    pred_f, _, frozen = frozen_oracle_step("superres", sd, names, *batch)
    pred_b, _, batchstat = frozen_oracle_step("superres", sd, names, *batch, training=True)
    with pytest.raises(AssertionError):
        check_grads(batchstat, frozen, REL_L2_F32, MAX_REL_F32, "batch statistics against frozen")
    errs, _ = grad_errors(batchstat, frozen)
    beyond = [n for n, (e_max, e_l2) in errs.items() if e_l2 > 100 * REL_L2_F32]
    print(f"{len(beyond)} of {len(errs)} tensors beyond 100x the bar; predictions {((pred_f - pred_b).norm() / pred_f.norm()).item():.2e} apart")
    assert len(beyond) > len(errs) // 2
    assert ((pred_f - pred_b).norm() / pred_f.norm()).item() > 100 * 1e-4
    # the frozen oracle is the oracle's own eval forward
    from oracle import unet_oracle as U
    with torch.no_grad():
        want = U.unet_forward(sd, batch[0], batch[1], batch[2], 2)
    assert ((pred_f.float() - want).abs().max() / want.abs().max()).item() < 1e-4
