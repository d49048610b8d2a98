"""Sampling with known pixels, host side (no GPU): the move schedule, the float64 oracle of tests/inpaint_oracle.py checked
against a perfect denoiser, the argument checks, the command-line flags, the seeded block masks and the chain driver's
roll-back over a list of moves."""
import math

import pytest
import torch

import inpaint_oracle as I
from oracle import diffusion_oracle as D


# ---------------------------------------------------------------------------------------------
# the schedule
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 7, 10, 49])
@pytest.mark.parametrize("resample", [1, 2, 3])
@pytest.mark.parametrize("jump", [1, 2, 3, 10])
def test_schedule_properties(S, resample, jump):
    from diffusionremotesensing_amd.train_diffusion_superres import inpaint_schedule
    moves = inpaint_schedule(S, resample, jump)
    assert moves == I.schedule(S, resample, jump)
    # a connected walk from position 0 to position S over single moves down and jumps of `jump` up
    assert moves[0][0] == 0 and moves[-1][1] == S
    assert all(a[1] == b[0] for a, b in zip(moves, moves[1:]))
    assert all(q == p + 1 or q == p - jump for p, q in moves)
    assert all(0 <= p <= S and 0 <= q <= S for p, q in moves)
    down = [m for m in moves if m[1] > m[0]]
    up = [m for m in moves if m[1] < m[0]]
    blocks = (S - 1) // jump
    assert len(down) == S + (resample - 1) * jump * blocks
    assert len(up) == (resample - 1) * blocks
    # every jump up is followed by exactly `jump` moves down, back to where it started; none starts at position S (level 0)
    for k, (p, q) in enumerate(moves):
        if q < p:
            assert p != S and p % jump == 0
            block = moves[k + 1:k + 1 + jump]
            assert len(block) == jump and all(b == a + 1 for a, b in block) and block[-1][1] == p
    if resample == 1:
        assert moves == [(p, p + 1) for p in range(S)]
    # every position with p % jump == 0 strictly inside the walk is arrived at `resample` times
    arrivals = {}
    for p, q in down:
        arrivals[q] = arrivals.get(q, 0) + 1
    for p in range(1, S):
        if p % jump == 0:
            assert arrivals[p] == resample


# ---------------------------------------------------------------------------------------------
# the oracle against a perfect denoiser
# ---------------------------------------------------------------------------------------------
def _keyed_source(seed):
    def src(i, shape):
        return torch.randn(shape, generator=torch.Generator().manual_seed(seed * 100003 + i), dtype=torch.float64)
    return src


def _point_mass_case(kind, T):
    sched = D.schedule(kind, T)
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand((2, 3, 8, 8), generator=g, dtype=torch.float64)
    mask = (torch.rand((2, 1, 8, 8), generator=g) < 0.5).to(torch.uint8)
    ah = sched[1]

    def perfect_denoiser(x, t):  # the exact noise of x_t when the data distribution is the point mass at x0
        a = float(ah[t])
        return (x.double() - math.sqrt(a) * x0) / math.sqrt(1 - a)
    return sched, x0, mask, perfect_denoiser


@pytest.mark.parametrize("resample,jump", [(1, 1), (3, 2)])
def test_oracle_ddim_chain_returns_the_point_mass(resample, jump):
    """With eps = (x - sqrt(ah) x0) / sqrt(1 - ah) the eta = 0 DDIM move maps any x to sqrt(ah_p) x0 + sqrt(1 - ah_p) eps, and
    the known pixels (`known` = x0) sit on the same line: the chain ends at x0 everywhere, to 1e-9.  Cosine schedule, whose
    alpha_hat[0] is 1 (the linear one ends at alpha_hat[0] = 1 - 1e-4, a noised x0); the denoiser sees the float64 state."""
    T, S = 40, 10
    sched, x0, mask, eps_fn = _point_mass_case("cosine", T)
    out = I.chain(eps_fn, tuple(x0.shape), T, *sched, S, 0.0, _keyed_source(3), x0, mask, resample, jump,
                  model_dtype=torch.float64)
    assert (out - x0).abs().max().item() <= 1e-9


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_oracle_ancestral_chain_returns_known_on_the_mask(kind):
    T = 25
    sched, x0, mask, eps_fn = _point_mass_case(kind, T)
    known = x0.float()
    out = I.chain(eps_fn, tuple(x0.shape), T, *sched, None, 0.0, _keyed_source(4), known, mask, 2, 3)
    m = mask.bool().expand_as(out)
    assert torch.equal(out[m], known.double()[m])
    assert torch.isfinite(out).all() and not torch.equal(out[~m], known.double()[~m])


def test_oracle_single_moves():
    """The move is a select between the two closed forms, and the forward jump composes like single forward steps."""
    alpha, ah, beta = D.schedule("cosine", 50)
    g = torch.Generator().manual_seed(1)
    x, eps, z, known = (torch.randn((1, 2, 4, 4), generator=g, dtype=torch.float64) for _ in range(4))
    mask = torch.tensor([[1, 0, 0, 1]] * 4, dtype=torch.uint8).view(1, 1, 4, 4)
    out = I.move(x, eps, z, known, mask, 20, 12, ah, eta=0.5)
    m = mask.bool().expand_as(out)
    assert torch.equal(out[~m], I.O.step(x, eps, z, 20, 12, 0.5, ah)[~m])
    a, b = I.known_coefficients(12, ah)
    assert torch.equal(out[m], (a * known + b * z)[m])
    assert a * a + b * b == pytest.approx(1.0, abs=1e-15)
    assert torch.equal(I.move(x, eps, None, known, mask, 1, 0, ah, alpha=alpha, beta=beta)[m], known[m])
    # variance of the jump s -> t is that of the single steps: prod(alpha) = ah_t / ah_s
    A, B = I.renoise_coefficients(3, 9, ah)
    prod = math.prod(float(ah[k]) / float(ah[k - 1]) for k in range(4, 10))
    assert A * A == pytest.approx(prod, rel=1e-12) and A * A + B * B == pytest.approx(1.0, abs=1e-15)
    # the float64 ancestral step agrees with the fp32 expression of oracle.diffusion_oracle
    want = D.sampler_step(x.float(), eps.float(), z.float(), torch.tensor([7]), alpha, ah, beta)
    got = I.ancestral_step(x.float(), eps.float(), z.float(), 7, alpha, ah, beta)
    assert (got - want.double()).abs().max().item() <= 1e-5


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
def test_check_inpaint_args():
    from diffusionremotesensing_amd.train_diffusion_superres import check_inpaint_args
    shape = (2, 3, 8, 8)
    known, mask = torch.zeros(3, 8, 8), torch.zeros(8, 8, dtype=torch.bool)
    check_inpaint_args(shape, None, None)
    check_inpaint_args(shape, known, mask, 3, 2)
    for k in (known, torch.zeros(2, 3, 8, 8)):
        for m in (mask, torch.zeros(1, 8, 8), torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(2, 1, 8, 8),
                  torch.zeros(2, 3, 8, 8)):
            check_inpaint_args(shape, k, m)
    with pytest.raises(ValueError, match="known without known_mask"):
        check_inpaint_args(shape, known, None)
    with pytest.raises(ValueError, match="known_mask without known"):
        check_inpaint_args(shape, None, mask)
    for bad in (torch.zeros(3, 8, 7), torch.zeros(1, 8, 8), torch.zeros(3, 3, 8, 8), torch.zeros(8, 8)):
        with pytest.raises(ValueError, match="known .* does not broadcast"):
            check_inpaint_args(shape, bad, mask)
    for bad in (torch.zeros(8, 7), torch.zeros(2, 8, 8), torch.zeros(3, 1, 8, 8), torch.zeros(2, 2, 8, 8), torch.zeros(8)):
        with pytest.raises(ValueError, match="known_mask .* does not broadcast"):
            check_inpaint_args(shape, known, bad)
    for name in ("resample", "jump"):
        for bad in (0, -1, 1.5, "2", None, True):
            with pytest.raises(ValueError, match=name + " must be an integer >= 1"):
                check_inpaint_args(shape, known, mask, **{name: bad})
        with pytest.raises(ValueError, match="belong to a chain with known pixels"):
            check_inpaint_args(shape, None, None, **{name: 2})


@pytest.mark.parametrize("kind", ["superres", "sar", "gen"])
def test_sample_known_rejects_before_the_engine_is_touched(kind):
    """All three `sample_known` methods check the known-pixel arguments first: the model here has no engine at all."""
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen

    class NoEngine(torch.nn.Module):
        def hip_engine(self):
            raise AssertionError("the engine was touched")
    model = NoEngine()
    known, mask = torch.zeros(1, 8, 8), torch.ones(8, 8)
    if kind == "superres":
        d = sr.Diffusion("cosine", model, "/nonexistent/s.pt", noise_steps=10, device="cpu", magnification_factor=2, image_size=8)
        call = lambda kn, m, **k: d.sample_known(2, model, torch.zeros(1, 4, 4), kn, m, input_channels=1, **k)  # noqa: E731
    elif kind == "sar":
        d = sar.Diffusion("cosine", model, "/nonexistent/s.pt", noise_steps=10, device="cpu", image_size=8)
        call = lambda kn, m, **k: d.sample_known(2, model, torch.zeros(2, 8, 8), kn, m, NDVI_channels=1, **k)  # noqa: E731
    else:
        d = gen.Diffusion("cosine", model, "/nonexistent/s.pt", noise_steps=10, device="cpu", image_size=8)
        call = lambda kn, m, **k: d.sample_known(2, model, kn, m, target_class=torch.tensor([1, 2]),  # noqa: E731
                                                 input_channels=1, **k)
    with pytest.raises(ValueError, match="known without known_mask"):
        call(known, None)
    with pytest.raises(ValueError, match="known_mask without known"):
        call(None, mask)
    with pytest.raises(ValueError, match="does not broadcast"):
        call(torch.zeros(2, 8, 8), mask)
    with pytest.raises(ValueError, match="resample must be an integer"):
        call(known, mask, resample=0)
    with pytest.raises(ValueError, match="belong to a chain with known pixels"):
        call(None, None, jump=2)
    with pytest.raises(ValueError, match="needs known and known_mask"):
        call(None, None)


def test_sample_keeps_its_signature_and_sample_known_adds_the_four():
    """`sample` is the reference's call, unchanged; `sample_known` is the same call with known, known_mask after the
    conditioning and resample, jump among the keywords."""
    import inspect

    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for cls in (sr.Diffusion, sar.Diffusion, gen.Diffusion):
        plain = inspect.signature(cls.sample).parameters
        kn = inspect.signature(cls.sample_known).parameters
        assert not {"known", "known_mask", "resample", "jump"} & set(plain)
        assert set(kn) == set(plain) | {"known", "known_mask", "resample", "jump"}
        assert all(kn[k].default == plain[k].default for k in plain)
        assert kn["known"].default is inspect.Parameter.empty and kn["known_mask"].default is inspect.Parameter.empty
        assert (kn["resample"].default, kn["jump"].default) == (1, 1)


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
def test_known_flags_on_the_evaluate_command_line():
    """--resample / --jump / --known_fraction / --known_block belong to `evaluate`, the one command that has a known image to
    give; the parsers of the trainers and the tiler, which sample whole images, keep their flag sets."""
    from diffusionremotesensing_amd import Aggregation_Sampling as A
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as sar
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    from diffusionremotesensing_amd.generate_new_imgs import train_diffusion_generation as gen
    for task in evaluate.TASKS:
        p = evaluate.add_known_args(evaluate.evaluate_arg_parser(task))
        args = p.parse_args([])
        assert (args.resample, args.jump, args.known_fraction, args.known_block) == (1, 1, None, None)
        args = p.parse_args(["--resample", "3", "--jump", "2", "--known_fraction", "0.4", "--known_block", "8"])
        assert (args.resample, args.jump, args.known_fraction, args.known_block) == (3, 2, 0.4, 8)
    for p in (sr.build_arg_parser(), sar.train_arg_parser(), gen.build_arg_parser(), A.build_arg_parser()):
        assert not {"resample", "jump", "known_fraction", "known_block"} & {a.dest for a in p._actions}


def test_evaluate_refuses_known_flags_without_a_fraction(tmp_path, monkeypatch):
    from diffusionremotesensing_amd import evaluate
    monkeypatch.chdir(tmp_path)
    base = ["--task", "sar_to_ndvi", "--model_name", "m", "--image_size", "16", "--dataset_path", "synthetic:8"]
    for extra in (["--resample", "2"], ["--jump", "2"], ["--known_block", "4"], ["--known_fraction", "1.0"],
                  ["--known_fraction", "0"]):
        with pytest.raises(SystemExit):
            evaluate.main(base + extra)


def test_format_table_with_psnr_unknown():
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd.train_diffusion_superres import format_scores
    scores = {"model": {"psnr": 30.0, "ssim": 0.9, "psnr_unknown": 26.02}, "bicubic": {"psnr": 28.0, "ssim": 0.8}}
    table = evaluate.format_table(scores)
    assert "PSNR unknown" in table.splitlines()[0] and "26.02 dB" in table.splitlines()[1]
    assert table.splitlines()[2].split()[-1] == "-"
    assert "PSNR unknown 26.02 dB" in format_scores(scores)


# ---------------------------------------------------------------------------------------------
# block masks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,fraction,block", [(64, 0.4, 8), (32, 0.25, 5), (16, 0.0, 4), (20, 0.9, 7), (8, 1.0, 8)])
def test_block_mask(size, fraction, block):
    from diffusionremotesensing_amd import synthetic
    m = synthetic.block_mask("t.mask", 3, size, fraction, block, seed=1)
    assert m.shape == (3, 1, size, size) and m.dtype == torch.uint8 and set(m.unique().tolist()) <= {0, 1}
    assert torch.equal(m, synthetic.block_mask("t.mask", 3, size, fraction, block, seed=1))
    hidden = (m == 0).float().mean(dim=(1, 2, 3))
    assert ((hidden >= fraction - 1e-9) & (hidden < fraction + block * block / size ** 2 + 1e-9)).all(), hidden
    if 0 < fraction < 1:
        assert not torch.equal(m[0], m[1])  # one mask per image
        assert not torch.equal(m, synthetic.block_mask("t.mask", 3, size, fraction, block, seed=2))
        assert not torch.equal(m, synthetic.block_mask("t.other", 3, size, fraction, block, seed=1))
        # a union of block x block squares: every hidden pixel lies in a fully hidden square
        h = (m[:, 0] == 0).float()
        full = torch.nn.functional.avg_pool2d(h.unsqueeze(1), block, stride=1) == 1  # top-left corners of hidden squares
        cover = torch.nn.functional.conv_transpose2d(full.float(), torch.ones(1, 1, block, block)) > 0
        assert torch.equal(cover[:, 0], h.bool())
    with pytest.raises(ValueError):
        synthetic.block_mask("t.mask", 1, 8, 1.5, 2)
    with pytest.raises(ValueError):
        synthetic.block_mask("t.mask", 1, 8, 0.5, 9)


def test_psnr_masked_cpu_expression():
    from diffusionremotesensing_amd import metrics
    a = torch.zeros(2, 2, 4, 4)
    b = torch.zeros(2, 2, 4, 4)
    b[0, :, :2] = 0.5  # error 0.5 on the upper half of image 0
    b[1] = 3.0         # clamped to 1: error 1 everywhere
    where = torch.zeros(2, 1, 4, 4, dtype=torch.bool)
    where[:, :, :2] = True
    got = metrics.psnr_masked(a, b, where)
    assert got.dtype == torch.float64
    assert got[0].item() == pytest.approx(10 * math.log10(1 / 0.25)) and got[1].item() == pytest.approx(0.0)
    assert metrics.psnr_masked(a, b, ~where)[0].item() == math.inf


# ---------------------------------------------------------------------------------------------
# the chain driver over a list of moves
# ---------------------------------------------------------------------------------------------
def test_run_reverse_chain_rolls_back_to_a_position_in_the_move_list(capsys):
    from diffusionremotesensing_amd import _lib
    from diffusionremotesensing_amd.train_diffusion_superres import inpaint_schedule, run_reverse_chain
    moves = inpaint_schedule(7, 2, 3)  # 13 moves down, 2 up

    class Engine:
        def __init__(self, fail_at):
            self.checks, self.fail_at = 0, fail_at

        def check_faults(self):
            self.checks += 1
            if self.checks == self.fail_at:
                raise _lib.RangeFault("range")

    def run(fail_at):
        x, done, frames = torch.zeros(1), [], []

        def step(move):
            done.append(move)
            x.mul_(3).add_(move[0] * 10 + move[1])  # depends on the order of the moves
            frames.append(x.clone())
        eng = Engine(fail_at)
        run_reverse_chain(eng, x, 8, step, frames, every=4, timesteps=moves)
        return x, done, frames, eng
    x0, done0, frames0, _ = run(None)
    assert done0 == moves
    x1, done1, frames1, eng = run(2)  # the second check (after move 8) fails: moves 4 .. 7 run again
    assert done1 == moves[:8] + moves[4:]
    assert torch.equal(x0, x1) and len(frames1) == len(moves) and all(torch.equal(a, b) for a, b in zip(frames0, frames1))
    assert f"resuming the chain at step {moves[4]}" in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------
# the one move list of every chain kind
# ---------------------------------------------------------------------------------------------
# (t, t_to) at noise_steps = 8, written down from the three forms the samplers used to keep: range(T - 1, 0, -1) for the
# ancestral chain, the `ddim_timesteps` with their successors for DDIM, `inpaint_schedule` mapped onto the levels with known pixels
_DOWN7 = [(7, 6), (6, 5), (5, 4), (4, 3), (3, 2), (2, 1), (1, 0)]
CHAIN_MOVES_T8 = {
    # (sampling_steps, resample, jump)
    (None, 1, 1): _DOWN7,
    (1, 1, 1): [(7, 0)],
    (3, 1, 1): [(7, 4), (4, 1), (1, 0)],
    (7, 1, 1): _DOWN7,
    (None, 2, 1): [(7, 6), (6, 7), (7, 6), (6, 5), (5, 6), (6, 5), (5, 4), (4, 5), (5, 4), (4, 3), (3, 4), (4, 3), (3, 2), (2, 3),
                   (3, 2), (2, 1), (1, 2), (2, 1), (1, 0)],
    (None, 2, 2): [(7, 6), (6, 5), (5, 7), (7, 6), (6, 5), (5, 4), (4, 3), (3, 5), (5, 4), (4, 3), (3, 2), (2, 1), (1, 3), (3, 2),
                   (2, 1), (1, 0)],
    (None, 3, 2): [(7, 6), (6, 5), (5, 7), (7, 6), (6, 5), (5, 7), (7, 6), (6, 5), (5, 4), (4, 3), (3, 5), (5, 4), (4, 3), (3, 5),
                   (5, 4), (4, 3), (3, 2), (2, 1), (1, 3), (3, 2), (2, 1), (1, 3), (3, 2), (2, 1), (1, 0)],
    (3, 2, 1): [(7, 4), (4, 7), (7, 4), (4, 1), (1, 4), (4, 1), (1, 0)],
    (3, 2, 2): [(7, 4), (4, 1), (1, 7), (7, 4), (4, 1), (1, 0)],
    (3, 3, 2): [(7, 4), (4, 1), (1, 7), (7, 4), (4, 1), (1, 7), (7, 4), (4, 1), (1, 0)],
}


@pytest.mark.parametrize("key", list(CHAIN_MOVES_T8), ids=lambda k: f"S{k[0]}-r{k[1]}-j{k[2]}")
def test_chain_moves_are_the_three_former_step_lists(key):
    from diffusionremotesensing_amd.sampling import chain_moves
    sampling_steps, resample, jump = key
    moves = chain_moves(8, sampling_steps, resample, jump)
    assert moves == CHAIN_MOVES_T8[key] and all(type(t) is int and type(t_to) is int for t, t_to in moves)
    # the counts of `inpaint_schedule`'s docstring, none of the jumps up from level 0
    S = 7 if sampling_steps is None else sampling_steps
    down, up = [m for m in moves if m[1] < m[0]], [m for m in moves if m[1] > m[0]]
    assert len(down) == S + (resample - 1) * jump * ((S - 1) // jump) and len(up) == (resample - 1) * ((S - 1) // jump)
    assert len(down) + len(up) == len(moves) and all(t >= 1 for t, _ in up) and moves[-1][1] == 0
    # in the roll-back line of `run_reverse_chain` a move reads as the level it starts from
    assert f"{moves[0]}" == "7" and moves[0].t == 7 and moves[0].t_to == CHAIN_MOVES_T8[key][0][1]


def test_chain_moves_without_resampling_ignore_jump_and_check_the_steps():
    from diffusionremotesensing_amd.sampling import chain_moves
    assert chain_moves(8, None, 1, 3) == _DOWN7 and chain_moves(8) == _DOWN7
    with pytest.raises(ValueError, match="outside"):
        chain_moves(8, 8)
