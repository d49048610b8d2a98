"""The control flow of the three `Diffusion.sample` methods and the three trainers' CLI parsers, without a GPU.

The samplers run on device="cpu" over a fake model whose engine records every forward and returns a cheap deterministic
"eps", with logging stand-ins for the `hip_ops` update calls that still make the final x depend on every call.  Each case
is compared with a straight-line chain written out below (`_expect`): the ordered call log, the keys the noise source was
asked for (and between which updates), the train / eval state of the model, the frames of the video, and the final x, bit
for bit."""
import math
import os
import types

import pytest
import torch

T = 12  # noise_steps of most cases: the ancestral chain visits 11 .. 1
S = 4  # image size
VIDEO_MODULE = "diffusionremotesensing_amd.video"


# ---------------------------------------------------------------------------------------------
# the fake arithmetic: used by the stand-ins AND by the straight-line chain of the expectations
# ---------------------------------------------------------------------------------------------
def _eps(x, t, cond, labels):
    e = 0.5 * x + 0.01 * t.to(torch.float32).view(-1, 1, 1, 1)
    if cond is not None:
        e = e + 0.1 * cond.mean(dim=(1, 2, 3)).view(-1, 1, 1, 1)  # (1, ...) broadcasts over the chains, (n, ...) is per chain
    if labels is not None:
        e = e + 0.001 * labels.to(torch.float32).view(-1, 1, 1, 1)
    return e


def _ancestral(x, eps, noise, t):
    x.mul_(0.9).sub_(0.1 * eps).add_(0.001 * t)
    if noise is not None:
        x.add_(0.05 * noise)
    return x


def _ddim(x, eps, noise, t, t_prev, eta):
    x.mul_(0.7).sub_(0.2 * eps).add_(0.001 * t_prev + 0.01 * eta)
    if noise is not None:
        x.add_(0.03 * noise)
    return x


def _keyed_noise(i, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(1000 + i))


# ---------------------------------------------------------------------------------------------
# fakes
# ---------------------------------------------------------------------------------------------
class _Engine:
    def __init__(self, rec, fault_at=0):
        self.rec, self.fault_at, self.checks, self.model = rec, fault_at, 0, None

    def forward(self, x, t, cond, mag, **kw):
        assert set(kw) <= {"reuse_cond", "check_weights", "labels"}, kw
        labels = kw.get("labels")
        self.rec.log.append(("forward", tuple(x.shape), t.tolist(), None if cond is None else tuple(cond.shape), mag,
                             kw.get("reuse_cond"), kw.get("check_weights"), None if labels is None else labels.tolist()))
        self.rec.training.append(self.model.training)
        return _eps(x, t, cond, labels)

    def check_faults(self):
        self.checks += 1
        if self.checks == self.fault_at:
            from diffusionremotesensing_amd import _lib
            raise _lib.RangeFault("drs_unet_check_faults failed with status 6: test")


class _Net(torch.nn.Module):
    num_classes = 10

    def __init__(self, engine):
        super().__init__()
        self.engine = engine

    def hip_engine(self):
        return self.engine


class _Wrapped(torch.nn.Module):
    """What a data-parallel wrapper looks like to `sample`: `.module`, no `hip_engine`."""

    def __init__(self, net):
        super().__init__()
        self.module = net


class _Rec:
    def __init__(self):
        self.log, self.noise, self.training, self.updates = [], [], [], 0

    def source(self, i, shape):
        self.noise.append((i, tuple(shape), self.updates))
        return _keyed_noise(i, shape)


@pytest.fixture
def rec(monkeypatch):
    """Recording stand-ins for the hip_ops calls of a chain and for video.video_maker."""
    import sys

    from diffusionremotesensing_amd import hip_ops
    r = _Rec()
    r.schedules = None  # (alpha, alpha_hat, beta) of the Diffusion under test: the updates must be handed these very tensors

    def timestep_table(noise_steps, n, device):
        r.log.append(("timestep_table", noise_steps, n, str(torch.device(device))))
        return torch.arange(noise_steps, dtype=torch.int64).unsqueeze(1).expand(noise_steps, n).contiguous()

    def sampler_step_(x, eps_pred, noise, t, alpha, alpha_hat, beta):
        assert all(a is b for a, b in zip((alpha, alpha_hat, beta), r.schedules))
        r.log.append(("sampler_step_", t, noise is None))
        r.updates += 1
        return _ancestral(x, eps_pred, noise, t)

    def sampler_step_cfg_(x, eps_cond, eps_uncond, cfg_scale, noise, t, alpha, alpha_hat, beta):
        assert all(a is b for a, b in zip((alpha, alpha_hat, beta), r.schedules))
        r.log.append(("sampler_step_cfg_", cfg_scale, t, noise is None))
        r.updates += 1
        return _ancestral(x, torch.lerp(eps_uncond, eps_cond, float(cfg_scale)), noise, t)

    def ddim_step_(x, eps_cond, noise, t, t_prev, eta, alpha_hat, eps_uncond=None, cfg_scale=0.0):
        assert alpha_hat is r.schedules[1]
        r.log.append(("ddim_step_", t, t_prev, eta, noise is None, eps_uncond is None, cfg_scale))
        r.updates += 1
        eps = eps_cond if eps_uncond is None else torch.lerp(eps_uncond, eps_cond, float(cfg_scale))
        return _ddim(x, eps, noise, t, t_prev, eta)

    def video_maker(frames, path, fps):
        r.log.append(("video_maker", len(frames), path, fps))
        r.frames = [f.clone() for f in frames]

    for f in (timestep_table, sampler_step_, sampler_step_cfg_, ddim_step_):
        monkeypatch.setattr(hip_ops, f.__name__, f)
    monkeypatch.setitem(sys.modules, VIDEO_MODULE, types.SimpleNamespace(video_maker=video_maker))
    return r


def _make(kind, rec, noise_steps=T, fault_at=0, wrapped=False):
    """(diffusion, the model to hand to sample, engine) of one sampler on the CPU."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as GenDiffusion
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as SarDiffusion
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    engine = _Engine(rec, fault_at)
    net = _Net(engine)
    model = _Wrapped(net) if wrapped else net
    engine.model = model
    common = dict(noise_steps=noise_steps, device="cpu", image_size=S, model_name=f"host_{kind}")
    if kind == "superres":
        d = Diffusion("cosine", model, "/nonexistent/snapshot.pt", magnification_factor=2, Degradation_type="DownBlur", **common)
    else:
        d = (SarDiffusion if kind == "sar" else GenDiffusion)("cosine", model, "/nonexistent/snapshot.pt", **common)
        assert not hasattr(d, "magnification_factor") and not hasattr(d, "Degradation_type")
    rec.schedules = (d.alpha, d.alpha_hat, d.beta)
    assert model.training
    return d, model, engine


# ---------------------------------------------------------------------------------------------
# the expectation: one chain, written straight down
# ---------------------------------------------------------------------------------------------
def _timesteps(noise_steps, sampling_steps):
    if sampling_steps is None:
        return list(range(noise_steps - 1, 0, -1))
    if sampling_steps == 1:
        return [noise_steps - 1]
    return [1 + (k * (noise_steps - 2)) // (sampling_steps - 1) for k in range(sampling_steps)][::-1]


def _expect(kind, n, channels, sampling_steps, eta, draw, *, noise_steps=T, cond=None, mag=None, labels=None, cfg_scale=0,
            video_name=None, rerun=()):
    """(log, noise keys, final x, frames) of a chain.  `draw(i, shape)` supplies x_T (i = noise_steps) and the step noise;
    `labels` is what the engine is handed (2n entries = guided).  `rerun` lists (start, stop) positions of the timestep
    list that run a second time after a range fault: x is unchanged by a rollback + re-run with the same noise, the log is
    not."""
    shape = (n, channels, S, S)
    guided = labels is not None and len(labels) == 2 * n and kind == "gen" and cfg_scale > 0
    rows = 2 * n if kind == "gen" else n
    log = [("timestep_table", noise_steps, rows, "cpu")]
    keys, frames = [], []
    x = draw(noise_steps, shape).clone()
    keys.append((noise_steps, shape, 0))
    seq = _timesteps(noise_steps, sampling_steps)
    lab = None if labels is None else torch.tensor(labels, dtype=torch.int64)
    order = list(range(len(seq)))
    for a, b in rerun:
        order = order[:b] + list(range(a, b)) + order[b:]
    done = set()
    updates = 0
    for pos, k in enumerate(order):
        t = seq[k]
        t_prev = seq[k + 1] if k + 1 < len(seq) else 0
        first = pos == 0
        second_time = k in done
        done.add(k)
        if kind == "gen":
            fwd = ("forward", (2 * n if guided else n, channels, S, S), [t] * (2 * n if guided else n), None, 1, None, first,
                   labels)
        else:
            fwd = ("forward", shape, [t] * n, tuple(cond.shape), mag, not first, first, None)
        log.append(fwd)
        if sampling_steps is None:
            has_noise = t > 1
            log.append(("sampler_step_cfg_", cfg_scale, t, not has_noise) if guided else ("sampler_step_", t, not has_noise))
        else:
            has_noise = eta > 0 and t_prev > 0
            log.append(("ddim_step_", t, t_prev, eta, not has_noise, not guided, cfg_scale if guided else 0.0))
        if has_noise:
            keys.append((t, shape, updates))
        updates += 1
        if second_time:
            continue  # x and the frames are those of the first visit (rolled back, then the same again)
        tt = torch.full((n,), t, dtype=torch.int64)
        if guided:
            e2 = _eps(x.repeat(2, 1, 1, 1), torch.cat([tt, tt]), None, lab)
            eps = torch.lerp(e2[n:], e2[:n], float(cfg_scale))
        else:
            eps = _eps(x, tt, cond, lab)
        z = draw(t, shape) if has_noise else None
        if sampling_steps is None:
            _ancestral(x, eps, z, t)
        else:
            _ddim(x, eps, z, t, t_prev, eta)
        frames.append(x.clone())
    if video_name is not None:
        log.append(("video_maker", len(seq), os.path.join(os.getcwd(), "models_run", video_name, "results",
                                                           "video_denoising.mp4"), 100))
    return log, keys, x, frames


def _seeded_draw(seed):
    """The draws of a chain without a noise_source: torch's global CPU generator, x_T first, then one per noisy step."""
    torch.manual_seed(seed)
    return lambda i, shape: torch.randn(shape)


MODES = [pytest.param(None, 0.0, id="ancestral"), pytest.param(5, 0.0, id="ddim-eta0"), pytest.param(5, 0.5, id="ddim-eta0.5"),
         pytest.param(T - 1, 1.0, id="ddim-all-steps")]


def _check(rec, model, x, want, with_source):
    log, keys, want_x, _ = want
    assert rec.log == log
    assert rec.noise == (keys if with_source else [])
    assert model.training is True
    assert rec.training and not any(rec.training)  # eval() during every forward
    assert x.dtype == torch.float32 and x.is_contiguous() and torch.equal(x, want_x)


def test_the_expected_timestep_lists():
    assert _timesteps(T, None) == [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
    assert _timesteps(T, 5) == [11, 8, 6, 3, 1]
    assert _timesteps(T, T - 1) == _timesteps(T, None)


# ---------------------------------------------------------------------------------------------
# A. the chains
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_source", [True, False], ids=["noise_source", "global-rng"])
@pytest.mark.parametrize("sampling_steps,eta", MODES)
def test_superres_chain(rec, sampling_steps, eta, with_source):
    d, model, _ = _make("superres", rec, wrapped=sampling_steps == 5)
    lr = torch.linspace(0, 1, 3 * 2 * 2).view(3, 2, 2)
    if with_source:
        x = d.sample(2, model, lr, 3, False, rec.source, sampling_steps, eta)  # the positional order is public
        draw = _keyed_noise
    else:
        torch.manual_seed(5)
        x = d.sample(2, model, lr, sampling_steps=sampling_steps, eta=eta)
        draw = _seeded_draw(5)
    _check(rec, model, x, _expect("superres", 2, 3, sampling_steps, eta, draw, cond=lr.unsqueeze(0), mag=2), with_source)


def test_superres_one_lr_image_per_chain_and_wrong_batch(rec):
    d, model, _ = _make("superres", rec)
    lr = torch.linspace(0, 1, 3 * 5 * 2 * 2).view(3, 5, 2, 2)
    x = d.sample(3, model, lr, input_channels=5, noise_source=rec.source, sampling_steps=5, eta=0.5)
    _check(rec, model, x, _expect("superres", 3, 5, 5, 0.5, _keyed_noise, cond=lr, mag=2), True)

    rec.log.clear()
    with pytest.raises(RuntimeError, match="a batch of 3 LR images for n=2 chains"):
        d.sample(2, model, lr, input_channels=5, noise_source=rec.source)
    assert rec.log == [] and model.training is True  # nothing ran


def test_superres_checks_come_before_the_engine(rec):
    d, model, engine = _make("superres", rec)
    model.hip_engine = None  # touching it would raise TypeError
    d.Degradation_type = "other"
    with pytest.raises(ValueError, match="sampling_steps"):  # the DDIM arguments first ...
        d.sample(1, model, torch.zeros(3, 2, 2), sampling_steps=T)
    with pytest.raises(ValueError, match="degradation type"):  # ... then the degradation type
        d.sample(1, model, torch.zeros(3, 2, 2))
    assert rec.log == [] and rec.noise == []


@pytest.mark.parametrize("with_source", [True, False], ids=["noise_source", "global-rng"])
@pytest.mark.parametrize("sampling_steps,eta", MODES)
def test_sar_chain(rec, sampling_steps, eta, with_source):
    d, model, _ = _make("sar", rec, wrapped=sampling_steps is None)
    sar = torch.linspace(-1, 1, 2 * S * S).view(2, S, S)
    if with_source:
        x = d.sample(2, model, sar, 1, False, rec.source, sampling_steps, eta)
        draw = _keyed_noise
    else:
        torch.manual_seed(6)
        x = d.sample(2, model, sar, NDVI_channels=4, sampling_steps=sampling_steps, eta=eta)
        draw = _seeded_draw(6)
    _check(rec, model, x, _expect("sar", 2, 1 if with_source else 4, sampling_steps, eta, draw, cond=sar.unsqueeze(0), mag=1),
           with_source)


GEN_LABELS = [  # (target_class, cfg_scale, n, the labels the engine must be handed)
    pytest.param([3, 7], 3, 2, [3, 7, -1, -1], id="class-cfg3"),
    pytest.param([3, 7], 0, 2, [3, 7], id="class-cfg0"),
    pytest.param(None, 3, 2, None, id="no-class"),
    pytest.param([4], 3, 3, [4, 4, 4, -1, -1, -1], id="one-class-for-3-chains"),
    pytest.param([4], 0, 3, [4], id="one-class-for-3-chains-cfg0"),
]


@pytest.mark.parametrize("target,cfg_scale,n,labels", GEN_LABELS)
@pytest.mark.parametrize("sampling_steps,eta", MODES)
def test_generation_chain(rec, sampling_steps, eta, target, cfg_scale, n, labels):
    d, model, _ = _make("gen", rec, wrapped=eta == 0.5)
    target = None if target is None else torch.tensor(target, dtype=torch.int64)
    x = d.sample(n, model, target, cfg_scale, 3, False, rec.source, sampling_steps, eta)
    _check(rec, model, x, _expect("gen", n, 3, sampling_steps, eta, _keyed_noise, labels=labels, cfg_scale=cfg_scale), True)


@pytest.mark.parametrize("sampling_steps,eta", MODES)
def test_generation_chain_global_rng_and_defaults(rec, sampling_steps, eta):
    d, model, _ = _make("gen", rec)
    torch.manual_seed(7)
    x = d.sample(2, model, target_class=torch.tensor([1, 2], dtype=torch.int32), sampling_steps=sampling_steps, eta=eta)
    want = _expect("gen", 2, 3, sampling_steps, eta, _seeded_draw(7), labels=[1, 2, -1, -1], cfg_scale=3)  # cfg_scale=3 default
    _check(rec, model, x, want, False)


def test_generation_class_out_of_range(rec):
    d, model, _ = _make("gen", rec)
    with pytest.raises(IndexError, match="target_class 10 out of range for num_classes=10"):
        d.sample(2, model, torch.tensor([1, 10]), noise_source=rec.source)
    with pytest.raises(IndexError, match="out of range"):
        d.sample(2, _Wrapped(model), torch.tensor([11]), cfg_scale=0)  # the class count is the wrapped network's
    assert rec.log == [] and rec.noise == []  # before x_T is drawn, before any forward


# ---------------------------------------------------------------------------------------------
# video frames, range faults
# ---------------------------------------------------------------------------------------------
def _run(kind, d, model, n, rec, **kw):
    if kind == "superres":
        lr = torch.linspace(0, 1, 3 * 2 * 2).view(3, 2, 2)
        return d.sample(n, model, lr, noise_source=rec.source, **kw), dict(cond=lr.unsqueeze(0), mag=2)
    if kind == "sar":
        sar = torch.linspace(-1, 1, 2 * S * S).view(2, S, S)
        return d.sample(n, model, sar, NDVI_channels=3, noise_source=rec.source, **kw), dict(cond=sar.unsqueeze(0), mag=1)
    out = d.sample(n, model, torch.tensor([5]), cfg_scale=2.5, noise_source=rec.source, **kw)
    return out, dict(labels=[5] * n + [-1] * n, cfg_scale=2.5)


@pytest.mark.parametrize("sampling_steps,eta", [(None, 0.0), (5, 0.5)], ids=["ancestral", "ddim"])
@pytest.mark.parametrize("kind", ["superres", "sar", "gen"])
def test_generate_video(rec, kind, sampling_steps, eta):
    d, model, _ = _make(kind, rec)
    x, extra = _run(kind, d, model, 2, rec, generate_video=True, sampling_steps=sampling_steps, eta=eta)
    want = _expect(kind, 2, 3, sampling_steps, eta, _keyed_noise, video_name=f"host_{kind}", **extra)
    _check(rec, model, x, want, True)
    assert len(rec.frames) == len(want[3]) == (T - 1 if sampling_steps is None else 5)
    assert all(torch.equal(a, b) for a, b in zip(rec.frames, want[3]))  # x after every step, copies (not views of x)
    assert torch.equal(rec.frames[-1], x)


@pytest.mark.parametrize("kind,sampling_steps,eta,fault_at,rerun", [
    # 139 ancestral steps, the fault word is read after 128 of them and at the end.  The first read faults: the chain goes
    # back to its start and runs the 128 again
    ("superres", None, 0.0, 1, (0, 128)),
    # the read at the end faults: back to the checkpoint after 128, the last 11 again
    ("sar", None, 0.0, 2, (128, 139)),
    ("gen", None, 0.0, 1, (0, 128)),
    # a DDIM chain of 130 of the 139 timesteps, eta > 0
    ("gen", 130, 0.5, 2, (128, 130)),
    ("superres", 130, 0.5, 1, (0, 128)),
])
def test_range_fault_in_mid_chain(rec, capsys, kind, sampling_steps, eta, fault_at, rerun):
    NT = 140
    d, model, engine = _make(kind, rec, noise_steps=NT, fault_at=fault_at)
    x, extra = _run(kind, d, model, 1, rec, generate_video=True, sampling_steps=sampling_steps, eta=eta)
    want = _expect(kind, 1, 3, sampling_steps, eta, _keyed_noise, noise_steps=NT, video_name=f"host_{kind}", rerun=[rerun],
                   **extra)
    _check(rec, model, x, want, True)
    steps = NT - 1 if sampling_steps is None else sampling_steps
    assert len(rec.frames) == steps  # the frames of the rolled-back steps were dropped
    assert all(torch.equal(a, b) for a, b in zip(rec.frames, want[3]))
    assert engine.checks == 3
    # "first" is the first call of the chain, not the first after a rollback
    forwards = [e for e in rec.log if e[0] == "forward"]
    assert len(forwards) == steps + rerun[1] - rerun[0]
    assert [e[6] for e in forwards] == [True] + [False] * (len(forwards) - 1)
    assert f"resuming the chain at step {_timesteps(NT, sampling_steps)[rerun[0]]}" in capsys.readouterr().err


def test_public_names_and_signatures():
    import inspect

    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    tail = [("generate_video", False), ("noise_source", None), ("sampling_steps", None), ("eta", 0.0)]
    assert sig(sr.Diffusion.sample) == [("self", E), ("n", E), ("model", E), ("lr_img", E), ("input_channels", 3)] + tail
    assert sig(sar.Diffusion.sample) == [("self", E), ("n", E), ("model", E), ("SAR_img", E), ("NDVI_channels", 1)] + tail
    assert sig(gen.Diffusion.sample) == [("self", E), ("n", E), ("model", E), ("target_class", None), ("cfg_scale", 3),
                                         ("input_channels", 3)] + tail
    assert sr.CHAIN_CHECK_EVERY == 128
    assert sig(sr.run_reverse_chain) == [("engine", E), ("x", E), ("noise_steps", E), ("step", E), ("frames", None),
                                         ("every", 128), ("timesteps", None)]
    assert sig(sr.ddim_timesteps) == [("noise_steps", E), ("sampling_steps", E)]
    assert sig(sr.check_sampling_args) == [("noise_steps", E), ("sampling_steps", E), ("eta", E)]
    assert sig(sr.ddim_chain_noise) == [("eta", E), ("t", E), ("t_prev", E), ("shape", E), ("x", E), ("noise_source", E)]
    assert sig(sr.add_sampling_args) == [("p", E)]


# ---------------------------------------------------------------------------------------------
# B. the parsers
# ---------------------------------------------------------------------------------------------
BOOL = "str2bool"
# option: (type, default, nargs, const)
COMMON_FLAGS = {
    "--epochs": (int, 501, None, None),
    "--batch_size": (int, 32, None, None),
    "--image_size": (int, None, None, None),
    "--lr": (float, 3e-4, None, None),
    "--check_preds_epoch": (int, 20, None, None),
    "--noise_schedule": (str, "cosine", None, None),
    "--snapshot_name": (str, "snapshot.pt", None, None),
    "--model_name": (str, None, None, None),
    "--noise_steps": (int, 200, None, None),
    "--patience": (int, 10, None, None),
    "--dataset_path": (str, None, None, None),
    "--generate_video": (BOOL, False, "?", True),
    "--loss": (str, None, None, None),
    "--UNet_type": (str, "Residual Attention UNet", None, None),
    "--multiple_gpus": (BOOL, False, "?", True),
    "--ema_smoothing": (BOOL, False, "?", True),
    "--sampling_steps": (int, None, None, None),
    "--eta": (float, 0.0, None, None),
}
OWN_FLAGS = {
    "train_diffusion_superres": {
        "--inp_out_channels": (int, 3, None, None),
        "--magnification_factor": (int, None, None, None),
        "--Degradation_type": (str, "DownBlur", None, None),
        "--num_crops": (int, 1, None, None),
        "--Blur_radius": (str, "random", None, None),
    },
    "train_diffusion_SAR_TO_NDVI": {
        "--SAR_channels": (int, 2, None, None),
        "--NDVI_channels": (int, 1, None, None),
    },
    "generate_new_imgs.train_diffusion_generation": {
        "--inp_out_channels": (int, 3, None, None),
    },
}


@pytest.mark.parametrize("name", sorted(OWN_FLAGS))
def test_parser_flags(name):
    import argparse
    import importlib
    p = importlib.import_module("diffusionremotesensing_amd." + name).build_arg_parser()
    want = {**COMMON_FLAGS, **OWN_FLAGS[name]}
    actions = [a for a in p._actions if not isinstance(a, argparse._HelpAction)]
    assert all(len(a.option_strings) == 1 for a in actions)
    got = {a.option_strings[0]: a for a in actions}
    assert len(got) == len(actions)
    assert set(got) == set(want)
    assert {s for a in p._actions for s in a.option_strings} == set(want) | {"-h", "--help"}
    for flag, (typ, default, nargs, const) in want.items():
        a = got[flag]
        assert type(a) is argparse._StoreAction and a.dest == flag[2:] and not a.required and a.choices is None, flag
        if typ == BOOL:
            assert [a.type(s) for s in ("yes", "True", "t", "1", "TRUE", "no", "false", "0", "", "y")] == [True] * 5 + [False] * 5
        else:
            assert a.type is typ, flag
        assert a.default == default and type(a.default) is type(default), flag
        assert a.nargs == nargs and a.const == const and a.const is const, flag
    args = p.parse_args(["--generate_video", "--multiple_gpus", "no", "--lr", "1e-3"])
    assert args.generate_video is True and args.multiple_gpus is False and args.ema_smoothing is False
    assert args.lr == 1e-3 and math.isclose(p.parse_args([]).lr, 3e-4)
