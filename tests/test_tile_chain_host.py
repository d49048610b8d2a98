"""Per-step tile aggregation without a GPU: the float64 oracle of the joint chain (tests/tile_chain_oracle.py) checked
against the single-image oracles it must reduce to, the tiler's argument checks, the CLI flag and the host-side validation of
drs_gather_tiles / drs_blend_step / drs_blend_step_ddim through the library."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import ddim_oracle as O
import tile_chain_oracle as TC
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D

T = 12
CH = 2


def _eps_fn(x_tiles, t, rng):
    """A cheap deterministic stand-in for the UNet: a fixed 3x3 convolution of x plus a function of t (fp32, per tile,
    the same function for every tile, one tile per call: a convolution's fp32 sums may depend on the batch size)."""
    k = torch.tensor([[0.05, -0.1, 0.02], [0.2, 0.4, -0.15], [0.0, 0.1, -0.05]])
    w = torch.stack([torch.stack([k, -0.5 * k]), torch.stack([0.3 * k.t(), k])])  # (2, 2, 3, 3)
    return torch.cat([F.conv2d(x1[None].float(), w, padding=1) for x1 in x_tiles]) + 0.1 * torch.sin(torch.tensor(0.37 * t))


def _scene_noise(seed, shape):
    """noise_source(i, shape) with one fixed draw per i: the same tensor whoever asks, so slices of it can drive tiles."""
    draws = {}

    def src(i, shp):
        assert tuple(shp) == tuple(shape), (shp, shape)
        if i not in draws:
            draws[i] = torch.randn(shape, generator=torch.Generator().manual_seed(seed * 10007 + i))
        return draws[i]
    return src


CHAINS = [("cosine", None, 0.0), ("linear", None, 0.0), ("cosine", 5, 0.0), ("cosine", 5, 1.0), ("linear", 4, 0.5)]


@pytest.mark.parametrize("kind,S,eta", CHAINS)
def test_one_tile_scene_is_the_single_image_chain(kind, S, eta):
    """A scene one tile covers: the blend is the identity and the joint chain is exactly `ddim_oracle.chain` / the ancestral
    oracle chain (diffusion_oracle.sampler_step on a float64 state) with the same noise."""
    sched = D.schedule(kind, T)
    infos, _ = A.tile_infos(8, 8, 8, 8, 2)
    assert infos == [(0, 16, 0, 16)]
    shape = (1, CH, 16, 16)
    got = TC.chain(_eps_fn, CH, 16, 16, infos, A.gaussian_weight(16, 16), T, sched, _scene_noise(3, shape), S, eta)
    if S is not None:
        want = O.chain(lambda x, t: _eps_fn(x, t, (0, 1)), shape, T, sched[1], S, eta, _scene_noise(3, shape))[0]
    else:
        src = _scene_noise(3, shape)
        x = src(T, shape).double()
        for i in range(T - 1, 0, -1):
            z = src(i, shape).double() if i > 1 else torch.zeros(shape, dtype=torch.float64)
            x = D.sampler_step(x, _eps_fn(x.float(), i, (0, 1)).double(), z, torch.full((1,), i), sched[0].double(),
                               sched[1].double(), sched[2].double())
        want = x[0]
    assert got.dtype == torch.float64
    assert torch.equal(got, want)


@pytest.mark.parametrize("kind,S,eta", CHAINS)
def test_partition_layout_equals_independent_tile_chains(kind, S, eta):
    """stride == patch_size on a scene the tiles partition: every scene element has one tile, so the joint chain equals the
    independent per-tile chains driven by the matching slices of the scene noise (float64, to 1e-12)."""
    sched = D.schedule(kind, T)
    h, w, ps, m = 16, 24, 8, 2
    infos, _ = A.tile_infos(h, w, ps, ps, m)
    assert len(infos) == 6
    shape = (1, CH, h * m, w * m)
    src = _scene_noise(5, shape)
    got = TC.chain(_eps_fn, CH, h * m, w * m, infos, A.gaussian_weight(ps * m, ps * m), T, sched, src, S, eta)
    for k, (y0, y1, x0, x1) in enumerate(infos):
        want = TC.tile_chain(_eps_fn, k, CH, ps * m, T, sched,
                             lambda i, shp, y0=y0, y1=y1, x0=x0, x1=x1: src(i, shape)[:, :, y0:y1, x0:x1], S, eta)
        err = (got[:, y0:y1, x0:x1] - want).abs().max().item()
        assert err <= 1e-12 * max(1.0, want.abs().max().item()), (k, err)


@pytest.mark.parametrize("kind,S,eta", CHAINS[:1] + CHAINS[2:3])
def test_overlapping_layout_differs_from_independent_tile_chains(kind, S, eta):
    """With overlap the joint chain is NOT the independent chains: the test scene really exercises the blend."""
    sched = D.schedule(kind, T)
    h, w, ps, st, m = 16, 24, 8, 4, 2
    infos, _ = A.tile_infos(h, w, ps, st, m)
    assert len(infos) == 15
    shape = (1, CH, h * m, w * m)
    src = _scene_noise(7, shape)
    got = TC.chain(_eps_fn, CH, h * m, w * m, infos, A.gaussian_weight(ps * m, ps * m), T, sched, src, S, eta)
    y0, y1, x0, x1 = infos[6]  # an interior tile: every element of it is shared with a neighbour
    want = TC.tile_chain(_eps_fn, 6, CH, ps * m, T, sched, lambda i, shp: src(i, shape)[:, :, y0:y1, x0:x1], S, eta)
    assert torch.isfinite(got).all()
    assert (got[:, y0:y1, x0:x1] - want).abs().max().item() > 1e-3


def test_oracle_blend_is_the_weighted_mean():
    infos, _ = A.tile_infos(8, 12, 8, 4, 1)
    wt = A.gaussian_weight(8, 8)
    e = torch.randn((len(infos), 1, 8, 8), generator=torch.Generator().manual_seed(1))
    got = TC.blend(e, infos, wt, 8, 12)
    num = torch.zeros((1, 8, 12), dtype=torch.float64)
    den = torch.zeros((8, 12), dtype=torch.float64)
    for k, (y0, y1, x0, x1) in enumerate(infos):
        num[:, y0:y1, x0:x1] += wt.double() * e[k].double()
        den[y0:y1, x0:x1] += wt.double()
    assert (got - num / den).abs().max().item() <= 1e-14
    const = TC.blend(torch.full_like(e, 0.75), infos, wt, 8, 12)  # a mean: constants are kept
    assert (const - 0.75).abs().max().item() <= 1e-15


@pytest.mark.parametrize("S", [None, 5])
def test_eta0_joint_chain_draws_only_x_T(S):
    """The noise protocol: an eta = 0 DDIM chain calls noise_source exactly once (x_T); the ancestral chain once per step
    but the last."""
    calls = []
    shape = (1, CH, 16, 16)

    def src(i, shp):
        calls.append((i, tuple(shp)))
        return torch.zeros(shp)
    infos, _ = A.tile_infos(8, 8, 8, 8, 2)
    TC.chain(_eps_fn, CH, 16, 16, infos, A.gaussian_weight(16, 16), T, D.schedule("cosine", T), src, S, 0.0)
    if S is not None:
        assert calls == [(T, shape)]
    else:
        assert calls == [(T, shape)] + [(i, shape) for i in range(T - 1, 1, -1)]


# ---------------------------------------------------------------------------------------------
# the tiler's argument checks (no engine, no GPU) and the CLI
# ---------------------------------------------------------------------------------------------
class _NoEngine(torch.nn.Module):
    def hip_engine(self):
        raise AssertionError("the engine must not be touched before the arguments are checked")


def _cpu_tiler():
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    m = _NoEngine()
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=20, device="cpu", magnification_factor=2,
                  image_size=16, Degradation_type="DownBlur")
    return split_aggregation_sampling(torch.zeros(1, 3, 8, 12), 8, 4, 2, d, "cpu")


def test_unknown_aggregation_raises_before_the_engine():
    tiler = _cpu_tiler()
    for bad in ("bogus", "", None, "PER_STEP"):
        with pytest.raises(ValueError, match="aggregation"):
            tiler.aggregation_sampling(aggregation=bad)
    for kw in ({"sampling_steps": 0}, {"sampling_steps": 20}, {"sampling_steps": 5, "eta": -1.0}):
        with pytest.raises(ValueError):
            tiler.aggregation_sampling(aggregation="per_step", **kw)
        with pytest.raises(ValueError):
            tiler.sample_scene(**kw)


def test_per_step_refuses_several_ranks(monkeypatch):
    """The joint chain is not sharded: under a process group of more than one rank it names the final mode instead."""
    from diffusionremotesensing_amd import dist
    tiler = _cpu_tiler()
    monkeypatch.setattr(dist, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="final"):
        tiler.aggregation_sampling(aggregation="per_step")
    with pytest.raises(NotImplementedError, match="final"):
        tiler.sample_scene(sampling_steps=5)


def test_aggregation_flag():
    from diffusionremotesensing_amd import Aggregation_Sampling
    p = Aggregation_Sampling.build_arg_parser()
    assert p.parse_args([]).aggregation == "final"
    assert p.parse_args(["--aggregation", "per_step"]).aggregation == "per_step"
    assert p.parse_args(["--aggregation", "final"]).aggregation == "final"
    with pytest.raises(SystemExit):
        p.parse_args(["--aggregation", "bogus"])


def test_launch_passes_the_aggregation_flag(monkeypatch, tmp_path):
    """`launch` hands --aggregation to the tiler (model, snapshot and chain replaced: no GPU)."""
    from diffusionremotesensing_amd import Aggregation_Sampling as AS
    from diffusionremotesensing_amd import UNet_model_superres, train_diffusion_superres
    seen = {}

    class FakeDiffusion:
        def __init__(self, **kw):
            self.model = kw["model"]

    def fake_sampling(self, noise_source=None, sampling_steps=None, eta=0.0, aggregation="final"):
        seen.update(aggregation=aggregation, sampling_steps=sampling_steps, eta=eta)
        return torch.zeros(1, 3, 16, 16)
    monkeypatch.setattr(train_diffusion_superres, "Diffusion", FakeDiffusion)
    monkeypatch.setattr(UNet_model_superres, "Residual_Attention_UNet_superres", lambda *a, **k: torch.nn.Identity())
    monkeypatch.setattr(AS.split_aggregation_sampling, "aggregation_sampling", fake_sampling)
    torch.save(torch.zeros(3, 8, 8), tmp_path / "lr.pt")
    argv = ["--model_name", "m", "--UNet_type", "Residual Attention UNet", "--Degradation_type", "DownBlur", "--device",
            "cpu", "--magnification_factor", "2", "--patch_size", "8", "--stride", "4", "--img_lr_path",
            str(tmp_path / "lr.pt"), "--destination_path", str(tmp_path / "out.pt")]
    for extra, want in (([], "final"), (["--aggregation", "per_step", "--sampling_steps", "7"], "per_step")):
        a = AS.build_arg_parser().parse_args(argv + extra)
        a.snapshot_folder_path = str(tmp_path)
        AS.launch(a)
        assert seen["aggregation"] == want
    assert seen["sampling_steps"] == 7


# ---------------------------------------------------------------------------------------------
# the C entry points: host-side validation, no launch
# ---------------------------------------------------------------------------------------------
def _host_ptr():
    buf = (C.c_float * 64)()  # host memory: every call below must fail validation before any launch
    return buf, C.cast(buf, C.c_void_p)


def test_blend_step_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf, p = _host_ptr()

    def anc(scene=p, eps=p, org=p, w=p, z=p, unc=None, n=2, Cc=1, S=4, Hs=4, Ws=8, t=10, a=p, ah=p, b=p, T=50):
        return lib.drs_blend_step(scene, eps, org, w, z, unc, n, Cc, S, Hs, Ws, t, a, ah, b, T, None)

    def ddim(scene=p, eps=p, org=p, w=p, z=p, unc=None, n=2, Cc=1, S=4, Hs=4, Ws=8, t=10, tp=5, eta=0.5, ah=p, T=50):
        return lib.drs_blend_step_ddim(scene, eps, org, w, z, unc, n, Cc, S, Hs, Ws, t, tp, eta, ah, T, None)

    ARG, SHAPE = 1, 2
    common = [({"scene": None}, ARG, b"null"), ({"eps": None}, ARG, b"null"), ({"org": None}, ARG, b"null"),
              ({"w": None}, ARG, b"null"), ({"ah": None}, ARG, b"null"), ({"S": 5}, SHAPE, b"S=5"),
              ({"S": 8, "Hs": 4, "Ws": 8}, SHAPE, b"S=8"), ({"S": 8, "Hs": 8, "Ws": 4}, SHAPE, b"S=8"),
              ({"n": 0}, SHAPE, b"n=0"), ({"Cc": 0}, SHAPE, b"C=0")]
    for fn, cases in ((anc, common + [({"a": None}, ARG, b"null"), ({"b": None}, ARG, b"null"), ({"t": 50}, ARG, b"t=50"),
                                      ({"t": -1}, ARG, b"t=-1")]),
                      (ddim, common + [({"tp": 10}, ARG, b"t_prev"), ({"tp": 11}, ARG, b"t_prev"), ({"tp": -1}, ARG, b"t_prev"),
                                       ({"t": 50}, ARG, b"t_prev"), ({"eta": -0.1}, ARG, b"eta"),
                                       ({"eta": float("nan")}, ARG, b"eta"), ({"eta": float("inf")}, ARG, b"eta"),
                                       ({"z": None}, ARG, b"noise")])):
        for kw, status, msg in cases:
            assert fn(**kw) == status, (fn.__name__, kw)
            assert msg in lib.drs_last_error(), (fn.__name__, kw, lib.drs_last_error())


def test_gather_tiles_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf, p = _host_ptr()

    def call(scene=p, org=p, tiles=p, first=0, count=2, n=2, Cc=1, S=4, Hs=4, Ws=8):
        return lib.drs_gather_tiles(scene, org, tiles, first, count, n, Cc, S, Hs, Ws, None)

    for kw, status in (({"scene": None}, 1), ({"org": None}, 1), ({"tiles": None}, 1), ({"first": 2}, 1), ({"first": -1}, 1),
                       ({"count": 0}, 1), ({"n": 0}, 1), ({"S": 5}, 2), ({"S": 8, "Ws": 4, "Hs": 8}, 2), ({"Cc": 0}, 2)):
        assert call(**kw) == status, kw
        assert b"gather_tiles" in lib.drs_last_error()


def test_tile_ops_have_no_cpu_fallback():
    from diffusionremotesensing_amd import hip_ops
    scene = torch.zeros(1, 8, 8)
    org = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.gather_tiles(scene, org, 8)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.blend_step_(scene, torch.zeros(1, 1, 8, 8), org, torch.ones(8, 8), None, 5, alpha_hat=torch.ones(10),
                            t_prev=2)
    with pytest.raises(RuntimeError, match="leaves"):
        hip_ops.tile_origins([(0, 4)], 8, 8, 8, "cpu")
    assert hip_ops.tile_origins([(0, 0), (0, 4)], 8, 8, 12, "cpu").tolist() == [[0, 0], [0, 4]]
