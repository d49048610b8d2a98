"""`sampling.sample_chain` on the GPU, without a UNet: the chain with its one step against the same chain written straight
down as explicit calls of the update wrappers, bit for bit, one case per branch of the step."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

T = 12
SHAPES = [(2, 3, 8, 8), (1, 1, 5, 7)]  # H * W = 35 is no multiple of 4: the scalar path of the known-pixel kernel
W_CFG = 3.0
DDIM4 = [(11, 7), (7, 4), (4, 1), (1, 0)]  # ddim_timesteps(12, 4) and their successors
# inpaint_schedule over the ancestral levels 11 .. 0 with resample = 2, jump = 2, and over DDIM4's with resample = 2, jump = 1
KNOWN_ANCESTRAL = [(11, 10), (10, 9), (9, 11), (11, 10), (10, 9), (9, 8), (8, 7), (7, 9), (9, 8), (8, 7), (7, 6), (6, 5), (5, 7),
                   (7, 6), (6, 5), (5, 4), (4, 3), (3, 5), (5, 4), (4, 3), (3, 2), (2, 1), (1, 3), (3, 2), (2, 1), (1, 0)]
KNOWN_DDIM = [(11, 7), (7, 11), (11, 7), (7, 4), (4, 7), (7, 4), (4, 1), (1, 4), (4, 1), (1, 0)]


@pytest.fixture(scope="module")
def schedule():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    dev = torch.device("cuda:0")
    steps = torch.arange(T) / T  # the cosine schedule of Diffusion.prepare_noise_schedule / from_alpha_hat_to_beta
    f_t = torch.cos(((steps + 0.008) / (1 + 0.008)) * torch.pi / 2) ** 2
    ah = (f_t / f_t[0]).to(dev)
    beta = torch.empty_like(ah)
    beta[0] = 1 - ah[0]
    beta[1:] = 1 - ah[1:] / ah[:-1]
    return types.SimpleNamespace(noise_steps=T, alpha=(1.0 - beta).contiguous(), alpha_hat=ah.contiguous(),
                                 beta=beta.contiguous(), device=dev)


class _Engine:
    def check_faults(self):
        pass


def _source(log):
    def source(i, shape):
        log.append((i, tuple(shape)))
        return torch.randn(shape, generator=torch.Generator().manual_seed(100 + i))
    return source


def _eps(x, guided):
    """The stand-in network: a deterministic function of x, a (cond, uncond) pair with guidance."""
    e = torch.sin(x * 1.5)
    return (e, torch.cos(x * 0.7)) if guided else e


def _known(shape, bands, dev):
    g = torch.Generator().manual_seed(5)
    known = torch.randn(shape, generator=g).to(dev)
    mask = (torch.rand((shape[0], bands) + shape[2:], generator=g) < 0.5).to(torch.uint8).to(dev)
    assert 0 < int(mask.sum()) < mask.numel()
    return known, mask


def _straight_down(s, shape, case, log):
    """The chain of `case` as explicit wrapper calls; the draws go through `_source(log)`."""
    from diffusionremotesensing_amd import hip_ops as H
    src = _source(log)
    x = src(T, shape).to(s.device).contiguous()
    z = lambda t: src(t, shape).to(s.device)  # noqa: E731
    if case == "ancestral":
        for i in range(T - 1, 0, -1):
            e = _eps(x, False)
            H.sampler_step_(x, e, z(i) if i > 1 else None, i, s.alpha, s.alpha_hat, s.beta)
    elif case == "ancestral-cfg":
        for i in range(T - 1, 0, -1):
            ec, eu = _eps(x, True)
            H.sampler_step_cfg_(x, ec, eu, W_CFG, z(i) if i > 1 else None, i, s.alpha, s.alpha_hat, s.beta)
    elif case == "ddim-eta0":
        for t, tp in DDIM4:
            H.ddim_step_(x, _eps(x, False), None, t, tp, 0.0, s.alpha_hat)
    elif case == "ddim-eta1-cfg":
        for t, tp in DDIM4:
            ec, eu = _eps(x, True)
            H.ddim_step_(x, ec, z(t) if tp > 0 else None, t, tp, 1.0, s.alpha_hat, eps_uncond=eu, cfg_scale=W_CFG)
    elif case == "known-ancestral":
        known, mask = _known(shape, shape[1], s.device)
        for t, to in KNOWN_ANCESTRAL:
            if to > t:
                H.renoise_(x, z(to), t, to, s.alpha_hat)
            else:
                e = _eps(x, False)
                H.inpaint_step_(x, e, z(t) if to > 0 else None, known, mask, t, alpha_hat=s.alpha_hat, alpha=s.alpha, beta=s.beta)
    else:
        assert case == "known-ddim"
        known, mask = _known(shape, 1, s.device)
        for t, to in KNOWN_DDIM:
            if to > t:
                H.renoise_(x, z(to), t, to, s.alpha_hat)
            else:
                e = _eps(x, False)
                H.inpaint_step_(x, e, z(t) if to > 0 else None, known, mask, t, alpha_hat=s.alpha_hat, t_prev=to, eta=0.5)
    return x


CASES = {  # the arguments `sample_chain` gets for the chain `_straight_down` writes out
    "ancestral": {},
    "ancestral-cfg": {"cfg_scale": W_CFG},
    "ddim-eta0": {"sampling_steps": 4, "eta": 0.0},
    "ddim-eta1-cfg": {"sampling_steps": 4, "eta": 1.0, "cfg_scale": W_CFG},
    "known-ancestral": {"resample": 2, "jump": 2},
    "known-ddim": {"sampling_steps": 4, "eta": 0.5, "resample": 2, "jump": 1},
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", list(CASES))
def test_sample_chain_equals_the_chain_written_straight_down(schedule, case, shape):
    from diffusionremotesensing_amd.sampling import sample_chain
    want_log, got_log, firsts = [], [], []
    want = _straight_down(schedule, shape, case, want_log)
    args = dict(CASES[case])
    guided = "cfg_scale" in args
    if case.startswith("known"):
        args["known"], args["known_mask"] = _known(shape, shape[1] if case == "known-ancestral" else 1, schedule.device)

    def predict(engine, x, t, first):
        assert t.shape == (shape[0],) and t.dtype == torch.int64
        firsts.append(first)
        return _eps(x, guided)
    frames = []
    got = sample_chain(schedule, _Engine(), shape, predict, table_rows=shape[0], noise_source=_source(got_log), frames=frames, **args)
    assert got_log == want_log and got_log[0] == (T, shape)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    assert firsts == [True] + [False] * (len(firsts) - 1)
    n_moves = {"ancestral": T - 1, "ancestral-cfg": T - 1, "ddim-eta0": 4, "ddim-eta1-cfg": 4,
               "known-ancestral": len(KNOWN_ANCESTRAL), "known-ddim": len(KNOWN_DDIM)}[case]
    assert len(frames) == n_moves and torch.equal(frames[-1], got)
