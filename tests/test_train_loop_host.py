"""What `Diffusion.train` prints, saves and leaves in `train_state` for scripted losses, and the three trainers' `--help`,
against transcripts recorded from the loop as it stood before it was split into steps (tests/golden/train_loop_transcripts.json;
`python tests/test_train_loop_host.py` records them again - only ever from a commit whose loop is known to be right).

The model is a `torch.nn.Linear` stub on the CPU: `train_step` returns scripted losses (and moves the weights, so that the raw
network and its EMA copy can be told apart), `noise_images` adds no noise and `_predict` returns a scripted constant v, which
makes the MSE validation loss v * v.  No run sets `max_grad_norm`: the clipping report needs a fused step on the device.
"""
import contextlib
import io
import json
import os
import sys
import tempfile
from unittest import mock

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "train_loop_transcripts.json")

RUNS = {
    # saves at epochs 0 and 1, early stopping at epoch 3
    "early_stop": dict(epochs=10, check_preds_epoch=1, patience=2, val_preds=(2.0, 1.0, 1.5, 1.25), ema_smoothing=False),
    # no validation: saves when epoch % check_preds_epoch == 0
    "no_val": dict(epochs=3, check_preds_epoch=2, patience=2, val_preds=None, ema_smoothing=False),
    "no_val_ema": dict(epochs=3, check_preds_epoch=2, patience=2, val_preds=None, ema_smoothing=True),
}


def _scripted_diffusion(folder, val_preds, ema_smoothing):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion

    class Scripted(Diffusion):
        train_losses = (1.0, 0.5)
        steps = 0
        preds = iter(val_preds or ())

        def train_step(self, model, optimizer, loss_function, lr_img, hr_img, ema=None, ema_model=None, lr_scheduler=None):
            with torch.no_grad():
                model.weight.add_(1.0)
            self.steps += 1
            return torch.tensor(self.train_losses[(self.steps - 1) % len(self.train_losses)])

        def noise_images(self, x, t):
            return x, torch.zeros_like(x)

        def _predict(self, net, x_t, t, cond):
            return torch.full_like(x_t, next(self.preds))

    model = torch.nn.Linear(3, 2)
    torch.nn.init.zeros_(model.weight)
    return Scripted("cosine", model, os.path.join(folder, "snapshot.pt"), noise_steps=10, device="cpu", magnification_factor=2,
                    image_size=8, Degradation_type="DownBlur", ema_smoothing=ema_smoothing)


def _run(folder, epochs, check_preds_epoch, patience, val_preds, ema_smoothing):
    """One scripted run in `folder`; everything the transcripts pin, as JSON-able values."""
    batch = (torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 8, 8))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        d = _scripted_diffusion(folder, val_preds, ema_smoothing)
        d.train(lr=1e-3, epochs=epochs, check_preds_epoch=check_preds_epoch, train_loader=[batch, batch],
                val_loader=[batch] if val_preds else None, patience=patience, loss="MSE", verbose=False)
    snapshot = torch.load(os.path.join(folder, "snapshot.pt"))
    return {"stdout": out.getvalue().replace(folder, "<folder>").splitlines(),
            "files": sorted(os.listdir(folder)),
            "epochs_run": snapshot["EPOCHS_RUN"],
            "snapshot_weight": sorted(set(snapshot["MODEL_STATE"]["weight"].flatten().tolist())),  # = train steps it has seen
            "best_loss": repr(d.train_state.best_loss),
            "epochs_without_improving": d.train_state.epochs_without_improving}


@contextlib.contextmanager
def _pinned_terminal():
    """argparse takes the program name from sys.argv[0] and the wrapping width from COLUMNS."""
    with mock.patch.dict(os.environ, {"COLUMNS": "100"}), mock.patch.object(sys, "argv", ["trainer"]):
        yield


def _help_texts():
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    out = io.StringIO()
    with _pinned_terminal():
        with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
            sr.parse_train_args(["--help"])
        return {"superres": out.getvalue().splitlines(), "sar": sar.train_main_parser().format_help().splitlines(),
                "generation": gen.train_main_parser().format_help().splitlines()}


def _expected():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(RUNS))
def test_scripted_run_matches_the_recorded_transcript(name, tmp_path):
    got, want = _run(str(tmp_path), **RUNS[name]), _expected()["runs"][name]
    assert got["stdout"] == want["stdout"]
    assert got == want


def test_early_stop_run_is_the_one_worked_out_by_hand(tmp_path):
    """The first transcript's figures, independent of the fixture: validation losses 4, 1, 2.25, 1.5625 with patience 2."""
    got = _run(str(tmp_path), **RUNS["early_stop"])
    saved = [line for line in got["stdout"] if "Training snapshot saved" in line]
    assert [line.split(" | ")[0] for line in saved] == ["Epoch 0", "Epoch 1"]
    assert got["stdout"][-1] == "Early stopping! Training stopped"
    assert "Epoch 3: Running Val loss (MSE)1.5625" in got["stdout"]
    assert (got["epochs_run"], got["best_loss"], got["epochs_without_improving"]) == (1, "1.0", 2)
    assert got["files"] == ["snapshot.pt"] and got["snapshot_weight"] == [4.0]


def test_ema_run_saves_the_ema_copy(tmp_path):
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    plain, ema = _run(str(tmp_path / "a"), **RUNS["no_val"]), _run(str(tmp_path / "b"), **RUNS["no_val_ema"])
    assert plain["epochs_run"] == ema["epochs_run"] == 2
    assert plain["snapshot_weight"] == [6.0]  # the raw network after the six steps of epochs 0 .. 2
    assert ema["snapshot_weight"] == [0.0]  # the copy made before the first step (the scripted step does not average into it)


@pytest.mark.parametrize("trainer", ["superres", "sar", "generation"])
def test_help_matches_the_recorded_text(trainer):
    assert _help_texts()[trainer] == _expected()["help"][trainer]


if __name__ == "__main__":
    record = {"runs": {}, "help": _help_texts()}
    for run_name, spec in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            record["runs"][run_name] = _run(tmp, **spec)
    with open(FIXTURE, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
