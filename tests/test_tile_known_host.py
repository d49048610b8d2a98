"""Known pixels in the tiler without a GPU: the argument checks of `split_aggregation_sampling` (raised before an engine
exists), the per-tile crops of the known scene and its mask, the command line, and the self-checks of the float64 oracle of
the joint chain with known pixels (tests/tile_known_oracle.py)."""
import pytest
import torch
import torch.nn.functional as F

import inpaint_oracle as I
import tile_known_oracle as TK
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D

T = 12
CH = 2
# (LR height, LR width, patch, stride, magnification) of the scenes of tests/test_gpu_tile_known.py (C1, C2, C3) and the seed
# of their block masks
LAYOUTS = {"one": (32, 32, 32, 32, 2), "sr": (48, 56, 32, 16, 2), "sar": (96, 112, 64, 32, 1)}
MASK_SEED = 1


def _eps_fn(x_tiles, t, rng):
    """The stand-in for the UNet of tests/test_tile_chain_host.py: a fixed 3x3 convolution of x plus a function of t."""
    k = torch.tensor([[0.05, -0.1, 0.02], [0.2, 0.4, -0.15], [0.0, 0.1, -0.05]])
    w = torch.stack([torch.stack([k, -0.5 * k]), torch.stack([0.3 * k.t(), k])])  # (2, 2, 3, 3)
    return torch.cat([F.conv2d(x1[None].float(), w, padding=1) for x1 in x_tiles]) + 0.1 * torch.sin(torch.tensor(0.37 * t))


def _replay(seed):
    gen = torch.Generator().manual_seed(seed)
    return lambda i, shape: torch.randn(shape, generator=gen)


class _NoEngine:
    """A Diffusion that has no engine: whatever gets past the argument checks fails with AttributeError, not ValueError."""
    model = None
    noise_steps = T
    image_size = 8


def _tiler(h=16, w=24, ps=8, st=4, m=2, channels=CH, d=None, **kw):
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    return split_aggregation_sampling(torch.zeros((1, channels, h, w)), ps, st, m, d or _NoEngine(), "cpu", **kw)


# ---------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["sample_scene", "sample_tiles", "aggregation_sampling", "aggregation_sampling/per_step"])
def test_known_pixel_requests_are_refused_before_the_engine(entry):
    from diffusionremotesensing_amd.sampling import sampling_plan
    tiler = _tiler()
    name, _, mode = entry.partition("/")
    extra = {"aggregation": mode} if mode else {}

    def call(**kw):
        return getattr(tiler, name)(**extra, **kw)
    Hs, Ws = 32, 48
    known, mask = torch.zeros((CH, Hs, Ws)), torch.zeros((Hs, Ws), dtype=torch.bool)
    for bad in (torch.zeros((CH, Hs, Ws + 1)), torch.zeros((CH + 1, Hs, Ws)), torch.zeros((1, CH, Hs, Ws)), torch.zeros((Hs, Ws))):
        with pytest.raises(ValueError, match="known"):
            call(known=bad, known_mask=mask)
    for bad in (torch.zeros((Hs + 1, Ws)), torch.zeros((3, Hs, Ws)), torch.zeros((1, 1, Hs, Ws)), torch.zeros((Ws,))):
        with pytest.raises(ValueError, match="known_mask"):
            call(known=known, known_mask=bad)
    with pytest.raises(ValueError, match="known without known_mask"):
        call(known=known)
    with pytest.raises(ValueError, match="known_mask without known"):
        call(known_mask=mask)
    with pytest.raises(ValueError, match="resample"):
        call(resample=2)
    with pytest.raises(ValueError, match="jump"):
        call(jump=2)
    with pytest.raises(ValueError, match="resample"):
        call(known=known, known_mask=mask, resample=0)
    with pytest.raises(ValueError, match="dpmpp_2m"):
        call(known=known, known_mask=mask, sampling_steps=sampling_plan(4, solver="dpmpp_2m"))
    for ok_mask in (mask, mask[None], mask[None].expand(CH, -1, -1)):  # the accepted shapes get past the checks
        with pytest.raises(AttributeError):
            call(known=known, known_mask=ok_mask, resample=2, jump=2)


def test_out_channels_and_clamp_arguments():
    t = _tiler()
    assert t.out_channels == CH and t.clamp == (0.0, 1.0)
    t = _tiler(out_channels=1, clamp=None)
    assert t.out_channels == 1 and t.clamp is None
    assert torch.equal(t._clamp(torch.tensor([-2.0, 3.0])), torch.tensor([-2.0, 3.0]))
    t = _tiler(clamp=(-1, 1))
    assert torch.equal(t._clamp(torch.tensor([-2.0, 0.5, 3.0])), torch.tensor([-1.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="clamp"):
        _tiler(clamp=(1.0, 0.0))
    with pytest.raises(ValueError, match="known"):  # the known scene has the sampled state's channels, not the conditioning's
        _tiler(out_channels=1).sample_scene(known=torch.zeros((CH, 32, 48)), known_mask=torch.zeros((32, 48)))


# ---------------------------------------------------------------------------------------------
# per-tile crops
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["sr", "sar"])
def test_known_tiles_are_the_windows_of_patches_sr_infos(layout):
    h, w, ps, st, m = LAYOUTS[layout]
    C = 3 if layout == "sr" else 1
    tiler = _tiler(h, w, ps, st, m, channels=3 if layout == "sr" else 2, out_channels=C)
    infos, _ = A.tile_infos(h, w, ps, st, m)
    assert [tuple(i) for i in tiler.patches_sr_infos] == infos and len(infos) == 6
    assert any(i[2] + ps * m == w * m and i[2] % (st * m) for i in infos)  # a clamped last tile off the stride grid
    Hs, Ws = h * m, w * m
    known = torch.arange(C * Hs * Ws, dtype=torch.float32).reshape(C, Hs, Ws)
    for mask in (TK.block_mask(MASK_SEED, Hs, Ws), TK.block_mask(MASK_SEED, Hs, Ws)[None],
                 torch.stack([TK.block_mask(MASK_SEED + c, Hs, Ws) for c in range(C)])):
        kn, mk = tiler.known_tiles(known, mask)
        m3 = mask if mask.dim() == 3 else mask[None]
        assert kn.shape == (6, C, ps * m, ps * m) and mk.shape == (6, m3.shape[0], ps * m, ps * m)
        for k, (y0, y1, x0, x1) in enumerate(infos):
            assert torch.equal(kn[k], known[:, y0:y1, x0:x1]) and torch.equal(mk[k], m3[:, y0:y1, x0:x1])


class _Recorder(_NoEngine):
    def __init__(self, S):
        self.image_size = S
        self.calls = []

    def sample(self, *a, **k):
        raise AssertionError("a chunk with known pixels is a sample_known call")

    def sample_known(self, n, model, lr, known, mask, channels, **kw):
        self.calls.append((n, lr.clone(), known.clone(), mask.clone(), channels, kw))
        if kw["noise_source"] is not None:
            kw["noise_source"](T, (n, channels, self.image_size, self.image_size))
        return torch.zeros((n, channels, self.image_size, self.image_size))


def test_sample_tiles_chunks_and_pads_the_crops_like_the_lr_tiles():
    """Six tiles in chunks of four: two `sample_known` calls of four chains, the second padded with repeats of the last tile -
    LR tile, known crop and mask crop alike - with the channel count passed positionally and resample / jump handed on."""
    h, w, ps, st, m = LAYOUTS["sar"]
    d = _Recorder(ps * m)
    tiler = _tiler(h, w, ps, st, m, channels=2, d=d, out_channels=1, clamp=None)
    tiler.img_lr.copy_(torch.rand(tiler.img_lr.shape))
    tiler.patches_lr, _ = tiler.patchifier(tiler.img_lr, ps, st, m)
    tiler.tile_batch = 4
    known = torch.rand((1, h, w))
    mask = TK.block_mask(MASK_SEED, h, w)
    asked = []

    def src(tile, i, shape):
        asked.append((tile, i, tuple(shape)))
        return torch.zeros(shape)
    out = tiler.sample_tiles(noise_source=src, sampling_steps=5, eta=0.5, known=known, known_mask=mask, resample=2, jump=3)
    assert out.shape == (6, 1, 64, 64)
    kn, mk = tiler.known_tiles(known, mask)
    lr = torch.cat([p[:1] for p in tiler.patches_lr])
    assert [c[0] for c in d.calls] == [4, 4]
    for (n, lr_c, kn_c, mk_c, channels, kw), idx in zip(d.calls, ([0, 1, 2, 3], [4, 5, 5, 5])):
        assert torch.equal(lr_c, lr[idx]) and torch.equal(kn_c, kn[idx]) and torch.equal(mk_c, mk[idx])
        assert channels == 1 and kw["resample"] == 2 and kw["jump"] == 3 and kw["sampling_steps"] == 5 and kw["eta"] == 0.5
    assert asked == [(k, T, (1, 1, 64, 64)) for k in range(6)]  # the padding repeats a draw, it does not ask for one


def test_masks_of_the_gpu_scenes_hold_both_kinds_in_every_tile():
    for name, (h, w, ps, st, m) in LAYOUTS.items():
        infos, _ = A.tile_infos(h, w, ps, st, m)
        frac = TK.check_mask(TK.block_mask(MASK_SEED, h * m, w * m), infos)
        assert 0.3 <= frac <= 0.7, (name, frac)


# ---------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------
def test_cli_flags_and_clamp_default():
    from diffusionremotesensing_amd.Aggregation_Sampling import build_arg_parser, cli_clamp
    p = build_arg_parser()
    a = p.parse_args([])
    assert (a.task, a.known_path, a.known_mask_path, a.known_resample, a.known_jump, a.clamp) == ("superres", None, None, 1, 1, None)
    assert (a.SAR_channels, a.NDVI_channels) == (2, 1)
    assert cli_clamp(a) == (0.0, 1.0)
    a = p.parse_args(["--task", "sar_to_ndvi", "--known_path", "k.pt", "--known_mask_path", "m.npy", "--resample", "3", "--jump",
                      "2", "--NDVI_channels", "2"])
    assert cli_clamp(a) is None and (a.known_resample, a.known_jump, a.NDVI_channels) == (3, 2, 2)
    assert cli_clamp(p.parse_args(["--task", "sar_to_ndvi", "--clamp=-1,1"])) == (-1.0, 1.0)
    assert cli_clamp(p.parse_args(["--clamp", "none"])) is None
    with pytest.raises(ValueError, match="clamp"):
        cli_clamp(p.parse_args(["--clamp", "1"]))
    with pytest.raises(SystemExit):
        p.parse_args(["--task", "generation"])


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------
CHAINS = [("cosine", None, 0.0, 1, 1), ("linear", None, 0.0, 2, 2), ("cosine", 5, 0.0, 1, 1), ("cosine", 5, 1.0, 2, 2),
          ("linear", 6, 0.5, 3, 2)]


@pytest.mark.parametrize("kind,S,eta,resample,jump", CHAINS)
def test_oracle_all_known_mask_returns_known(kind, S, eta, resample, jump):
    sched = D.schedule(kind, T)
    infos, _ = A.tile_infos(16, 24, 8, 4, 2)
    known = torch.randn((CH, 32, 48), generator=torch.Generator().manual_seed(1))
    got = TK.chain(_eps_fn, CH, 32, 48, infos, A.gaussian_weight(16, 16), T, sched, _replay(2), known,
                   torch.ones((32, 48), dtype=torch.bool), S, eta, resample, jump)
    assert got.dtype == torch.float64 and torch.equal(got, known.double())


@pytest.mark.parametrize("kind,S,eta,resample,jump", CHAINS)
def test_oracle_one_tile_scene_is_the_single_image_chain(kind, S, eta, resample, jump):
    """A scene one tile covers: the blend is the identity and the joint chain is `inpaint_oracle.chain` on that tile."""
    alpha, ah, beta = D.schedule(kind, T)
    infos, _ = A.tile_infos(8, 8, 8, 8, 2)
    assert infos == [(0, 16, 0, 16)]
    known = torch.randn((CH, 16, 16), generator=torch.Generator().manual_seed(3))
    mask = TK.block_mask(5, 16, 16, block=4)
    assert mask.any() and not mask.all()
    got = TK.chain(_eps_fn, CH, 16, 16, infos, A.gaussian_weight(16, 16), T, (alpha, ah, beta), _replay(4), known, mask, S,
                   eta, resample, jump)
    want = I.chain(lambda x, t: _eps_fn(x, t, (0, 1)), (1, CH, 16, 16), T, alpha, ah, beta, S, eta, _replay(4), known, mask,
                   resample, jump)
    assert torch.equal(got, want[0])
    assert torch.equal(got[mask[None].expand(CH, -1, -1)], known.double()[mask[None].expand(CH, -1, -1)])
    assert (got - known.double())[~mask[None].expand(CH, -1, -1)].abs().min().item() > 0


@pytest.mark.parametrize("kind,S,eta,resample,jump", CHAINS)
def test_oracle_moves_and_draws_are_those_of_chain_moves(kind, S, eta, resample, jump):
    from diffusionremotesensing_amd.sampling import chain_moves
    sched = D.schedule(kind, T)
    infos, _ = A.tile_infos(8, 12, 8, 4, 1)
    shape = (1, CH, 8, 12)
    asked, record = [], []

    def src(i, shp):
        assert tuple(shp) == shape
        asked.append(i)
        return torch.randn(shape, generator=torch.Generator().manual_seed(100 + len(asked)))
    TK.chain(_eps_fn, CH, 8, 12, infos, A.gaussian_weight(8, 8), T, sched, src, torch.zeros((CH, 8, 12)),
             TK.block_mask(2, 8, 12, block=4), S, eta, resample, jump, record=record)
    moves = chain_moves(T, S, resample, jump)
    assert [(t, t_to) for (_, t, t_to, _) in record] == [tuple(mv) for mv in moves]
    assert [kind_ for (kind_, *_rest) in record] == ["jump" if mv.t_to > mv.t else "move" for mv in moves]
    # x_T, then per move: a jump draws for the level it goes to, a reverse move for its t iff it ends above level 0
    assert asked == [T] + [mv.t_to if mv.t_to > mv.t else mv.t for mv in moves if mv.t_to > 0]
    assert [drew for (*_rest, drew) in record if drew is not None] == asked[1:]
