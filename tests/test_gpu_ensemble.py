"""Ensemble statistics and scores on the GPU (csrc/ensemble.hip through diffusionremotesensing_amd.ensemble) against the float64
oracle of tests/ensemble_oracle.py, `sample_ensemble` of the three models against `sample` calls made by hand, and
`Diffusion.evaluate(ensemble=N)` / the evaluate command."""
import json
import math

import pytest
import torch

import ensemble_oracle as EO
import metrics_oracle as MO
from conftest import replay_noise_source

pytestmark = pytest.mark.gpu

# One fp32 rounding of a result no larger than 2 M (M = the largest magnitude among the element's members and truth) is at
# most 2^-24 * 2 M; the bar is twice that.  Per-image sums: fewer than 1e4 elements times 2^-53, with margin.
TOL_MAP, TOL_SUM = 2.0 ** -22, 1e-12

SHAPES = [(1, 1, 7, 9),     # 63 elements: no group of four
          (2, 3, 16, 20),
          (2, 3, 40, 52)]   # several blocks per image, an image boundary inside the grid
MEMBER_COUNTS = [2, 3, 5, 8, 17, 32]  # both edges of every padding bucket
CLAMPS = [None, (0.0, 1.0)]
QUANTILE_LISTS = [(), (0.0, 1.0), (0.05, 0.5, 0.95), (0.0, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 1.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _case(shape, N, content, seed=0):
    """(members (N, B, C, H, W), truth (B, C, H, W)) fp32 CPU tensors: seeded Gaussians around 0.5 (the clamp to [0, 1] bites),
    or the same quantised to steps of 0.5 so that members tie with each other and with the truth (no negative zeros)."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * N + sum(shape) + (7 if content == "quantised" else 0))
    x = 0.5 + 0.6 * torch.randn((N,) + shape, generator=g)
    y = 0.5 + 0.6 * torch.randn(shape, generator=g)
    if content == "quantised":
        x, y = torch.round(x * 2) / 2 + 0.0, torch.round(y * 2) / 2 + 0.0
    return x, y


def _magnitude(x, y=None, clamp=None):
    """M per element: the largest magnitude among its (clamped) members and, when given, its truth."""
    x = x.double().clamp(*clamp) if clamp else x.double()
    m = x.abs().amax(dim=0)
    if y is not None:
        m = torch.maximum(m, (y.double().clamp(*clamp) if clamp else y.double()).abs())
    return m


def _map_ratio(got, want, M, what):
    """Worst |got - want| / (2^-22 M) of a map; asserts the bound element by element (M = 0: got == want)."""
    g = got.cpu()
    assert g.dtype == torch.float32 and g.shape == want.shape, what
    if g.numel() == 0:
        return 0.0
    d = (g.double() - want).abs()
    assert bool((d <= TOL_MAP * M.expand_as(d)).all()), (what, d.max().item())
    return (d / (TOL_MAP * M.expand_as(d)).clamp_min(1e-300)).max().item()


def _assert_sums(got, want, what):
    g = got.cpu()
    rel = ((g - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    assert rel <= TOL_SUM, (what, rel)
    return rel


@pytest.mark.parametrize("N", MEMBER_COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maps_and_sums_vs_float64_oracle(dev, shape, N):
    """Every map within 2^-22 M of the oracle, the per-image sums within 1e-12 relative, the rank histogram integer for
    integer; two contents, with and without the clamp, four quantile lists.  The worst ratios are printed."""
    from diffusionremotesensing_amd import hip_ops
    worst_map, worst_sum = 0.0, 0.0
    for content in ("gaussian", "quantised"):
        x, y = _case(shape, N, content)
        if content == "quantised" and x[0].numel() > 63:
            s = torch.sort(x, dim=0).values
            assert (s[1:] == s[:-1]).any() and (x == y).any()  # ties among members and with the truth do occur
        xd, yd = x.to(dev), y.to(dev)
        for clamp in CLAMPS:
            Mx, Mxy = _magnitude(x, None, clamp), _magnitude(x, y, clamp)
            for qs in QUANTILE_LISTS:
                mean, std, quant = hip_ops.ensemble_stats(xd, qs, clamp)
                want = EO.statistics(x, qs, clamp)
                what = (shape, N, content, clamp, qs)
                assert quant.shape == (len(qs),) + shape
                worst_map = max(worst_map, _map_ratio(mean, want["mean"], Mx, what), _map_ratio(std, want["std"], Mx, what),
                                _map_ratio(quant, want["quantiles"], Mx, what))
            sums, hist, crps = hip_ops.ensemble_scores(xd, yd, clamp, crps_map=True)
            worst_map = max(worst_map, _map_ratio(crps, EO.crps_map(x, y, clamp), Mxy, (shape, N, content, clamp, "crps")))
            assert sums.dtype == torch.float64 and hist.dtype == torch.int64
            worst_sum = max(worst_sum, _assert_sums(sums, EO.sums(x, y, clamp), (shape, N, content, clamp)))
            assert torch.equal(hist.cpu(), EO.rank_histogram(x, y, clamp))
            assert hist.sum(dim=1).tolist() == [shape[1] * shape[2] * shape[3]] * shape[0]
    print(f"ensemble {shape} N={N}: worst map error {worst_map:.3f} of the bound, worst sum error {worst_sum:.2e} relative")


def test_public_module_and_argument_errors(dev):
    from diffusionremotesensing_amd import ensemble, hip_ops
    x, y = _case((2, 3, 16, 20), 5, "gaussian")
    xd, yd = x.to(dev), y.to(dev)
    st = ensemble.ensemble_statistics(xd)
    want = EO.statistics(x, (0.05, 0.5, 0.95))
    assert set(st) == {"mean", "std", "quantiles"} and st["quantiles"].shape == (3, 2, 3, 16, 20)
    _map_ratio(st["quantiles"], want["quantiles"], _magnitude(x), "default quantiles")
    sc, want = ensemble.ensemble_scores(xd, yd, clamp=(0.0, 1.0)), EO.scores(x, y, (0.0, 1.0))
    assert set(sc) == {"crps", "spread", "rmse", "spread_skill", "rank_histogram"}
    for k in ("crps", "spread", "rmse", "spread_skill"):
        assert sc[k].dtype == torch.float64 and sc[k].shape == (2,)
        _assert_sums(sc[k], want[k], k)
    assert sc["rank_histogram"].shape == (2, 6) and torch.equal(sc["rank_histogram"].cpu(), want["rank_histogram"])
    # (N, C, H, W) members with a (C, H, W) truth: B = 1
    one = ensemble.ensemble_statistics(xd[:, 0].contiguous(), (0.5,))
    assert one["mean"].shape == (3, 16, 20) and one["quantiles"].shape == (1, 3, 16, 20)
    assert torch.equal(one["mean"], ensemble.ensemble_statistics(xd[:, :1].contiguous(), (0.5,))["mean"][0])
    sc1 = ensemble.ensemble_scores(xd[:, 0].contiguous(), yd[0])
    assert sc1["crps"].shape == (1,) and torch.equal(sc1["crps"], ensemble.ensemble_scores(xd, yd)["crps"][:1])
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.ensemble_stats(xd.transpose(3, 4))
    with pytest.raises(RuntimeError, match="float32"):
        hip_ops.ensemble_stats(xd.double())
    with pytest.raises(RuntimeError, match="2 <= N <= 32"):
        hip_ops.ensemble_stats(xd[:1])
    with pytest.raises(RuntimeError, match="truth"):
        hip_ops.ensemble_scores(xd, yd[:, :2])
    with pytest.raises(ValueError, match="quantiles"):
        hip_ops.ensemble_stats(xd, (0.5, 1.5))
    with pytest.raises(ValueError, match="clamp"):
        hip_ops.ensemble_stats(xd, clamp=(1.0, 0.0))


@pytest.mark.parametrize("N", MEMBER_COUNTS)
def test_identical_members_are_exact(dev, N):
    """N identical members: mean and every quantile are the member bit for bit, std is exactly 0, CRPS is the fp32 rounding of
    |x - y| and the spread sum exactly 0."""
    from diffusionremotesensing_amd import hip_ops
    x1, y = _case((2, 3, 16, 21), 2, "gaussian", seed=3)
    x = x1[:1].repeat(N, 1, 1, 1, 1).to(dev)
    mean, std, quant = hip_ops.ensemble_stats(x, QUANTILE_LISTS[3])
    assert torch.equal(mean, x[0]) and bool((std == 0).all())
    assert all(torch.equal(q, x[0]) for q in quant)
    sums, hist, crps = hip_ops.ensemble_scores(x, y.to(dev), crps_map=True)
    assert torch.equal(crps.cpu(), (x1[0].double() - y.double()).abs().float())
    assert bool((sums[:, 1] == 0).all())
    assert bool((hist[:, 1:N] == 0).all())  # the truth is below all members or above all of them


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_exact_properties(dev, shape):
    """q = 0 and q = 1 are amin and amax bit for bit; a permutation of the members changes no output bit; two calls are
    bit-identical; outputs requested alone equal the same outputs requested together."""
    from diffusionremotesensing_amd import hip_ops
    for N in MEMBER_COUNTS:
        for content in ("gaussian", "quantised"):
            x, y = _case(shape, N, content, seed=1)
            xd, yd = x.to(dev), y.to(dev)
            qs = (0.0, 1 / 3, 0.95, 1.0)
            mean, std, quant = hip_ops.ensemble_stats(xd, qs)
            sums, hist, crps = hip_ops.ensemble_scores(xd, yd, crps_map=True)
            assert torch.equal(quant[0], xd.amin(dim=0)) and torch.equal(quant[3], xd.amax(dim=0))
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(N))
            for members in (xd[perm.to(dev)].contiguous(), xd):  # permuted, then the same call again
                m2, s2, q2 = hip_ops.ensemble_stats(members, qs)
                sums2, hist2, crps2 = hip_ops.ensemble_scores(members, yd, crps_map=True)
                for a, b in ((mean, m2), (std, s2), (quant, q2), (sums, sums2), (hist, hist2), (crps, crps2)):
                    assert torch.equal(a, b), (N, content)
            only_mean = hip_ops.ensemble_stats(xd, None, std=False)
            only_std = hip_ops.ensemble_stats(xd, None, mean=False)
            only_q = hip_ops.ensemble_stats(xd, qs, mean=False, std=False)
            assert only_mean[1] is None and only_mean[2] is None and torch.equal(only_mean[0], mean)
            assert only_std[0] is None and torch.equal(only_std[1], std)
            assert only_q[0] is None and only_q[1] is None and torch.equal(only_q[2], quant)
            sums3, hist3, none = hip_ops.ensemble_scores(xd, yd)
            assert none is None and torch.equal(sums3, sums) and torch.equal(hist3, hist)


@pytest.mark.parametrize("where", ["member", "truth"])
def test_nan_stays_in_its_pixel_and_its_image(dev, where):
    from diffusionremotesensing_amd import hip_ops
    shape, N, qs = (2, 3, 16, 20), 5, (0.0, 0.5, 1.0)
    x, y = _case(shape, N, "gaussian", seed=2)
    clean_st = hip_ops.ensemble_stats(x.to(dev), qs)
    clean_sc = hip_ops.ensemble_scores(x.to(dev), y.to(dev), crps_map=True)
    at = (1, 2, 7, 13)
    if where == "member":
        x[(3,) + at] = float("nan")
    else:
        y[at] = float("nan")
    mean, std, quant = hip_ops.ensemble_stats(x.to(dev), qs)
    sums, hist, crps = hip_ops.ensemble_scores(x.to(dev), y.to(dev), crps_map=True)
    hole = torch.zeros(shape, dtype=torch.bool, device=dev)
    hole[at] = True
    maps = [(crps, clean_sc[2])]
    if where == "member":  # (the maps of ensemble_stats do not read the truth)
        maps += [(mean, clean_st[0]), (std, clean_st[1])] + list(zip(quant, clean_st[2]))
    else:
        assert all(torch.equal(a, b) for a, b in zip((mean, std, quant), clean_st))
    for got, clean in maps:
        assert math.isnan(got[at].item())
        assert torch.equal(got[~hole], clean[~hole])  # every other element bit-equal to the clean run
    assert bool(torch.isnan(sums[1]).all()) and torch.equal(sums[0], clean_sc[0][0])
    assert torch.equal(hist[0], clean_sc[1][0])
    assert hist[1].sum().item() == clean_sc[1][1].sum().item() - 1 and bool((hist[1] <= clean_sc[1][1]).all())


# ---------------------------------------------------------------------------------------------
# sample_ensemble
# ---------------------------------------------------------------------------------------------
T_STEPS, S_STEPS, SIZE, MAG = 8, 4, 64, 2


def _superres(dev, sd):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, magnification_factor=MAG,
                  image_size=SIZE, Degradation_type="DownBlur")
    return m, d


def _sar(dev, sd):
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    return m, Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, image_size=SIZE)


def _by_hand(sample, chunks, B):
    """The members of `chunks` direct sample calls, concatenated: (sum(chunks), B, C, S, S)."""
    x = torch.cat([sample(m) for m in chunks])
    return x.view(sum(chunks), B, *x.shape[1:])


def test_sample_ensemble_superres_is_three_sample_calls(dev, seeded_sd):
    """5 members of 2 LR images in chunks of 2 members = `sample` with 4, 4 and 2 chains on the repeated LR batch and the same
    draws, bit for bit (eta = 1: the source is asked at every step); with `known` every member keeps the known pixels."""
    from diffusionremotesensing_amd import synthetic
    m, d = _superres(dev, seeded_sd)
    lr = synthetic.tensor_uniform("ensemble.lr", (2, 3, SIZE // MAG, SIZE // MAG)).to(dev)
    got = d.sample_ensemble(5, m, lr, input_channels=3, member_batch=2, sampling_steps=S_STEPS, eta=1.0,
                            noise_source=replay_noise_source(51))
    src = replay_noise_source(51)
    want = _by_hand(lambda k: d.sample(2 * k, m, lr.repeat(k, 1, 1, 1), input_channels=3, noise_source=src,
                                       sampling_steps=S_STEPS, eta=1.0), [2, 2, 1], 2)
    assert got.shape == (5, 2, 3, SIZE, SIZE) and torch.equal(got, want)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0, 0], got[0, 1])
    known = synthetic.tensor_uniform("ensemble.known", (2, 3, SIZE, SIZE)).to(dev)
    mask = torch.zeros(SIZE, SIZE, dtype=torch.bool)
    mask[:, : SIZE // 2] = True
    kn = d.sample_ensemble(3, m, lr, input_channels=3, member_batch=2, sampling_steps=S_STEPS, noise_source=replay_noise_source(52),
                           known=known, known_mask=mask)
    assert kn.shape == (3, 2, 3, SIZE, SIZE)
    assert torch.equal(kn[..., : SIZE // 2], known[..., : SIZE // 2].expand(3, -1, -1, -1, -1))
    assert not torch.equal(kn[0, ..., SIZE // 2:], kn[1, ..., SIZE // 2:])


def test_sample_ensemble_sar_to_ndvi_is_three_sample_calls(dev, seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    m, d = _sar(dev, seeded_sd_sar)
    sar = synthetic.tensor_uniform("ensemble.sar", (2, 2, SIZE, SIZE)).to(dev)
    got = d.sample_ensemble(5, m, sar, NDVI_channels=1, member_batch=2, sampling_steps=S_STEPS, noise_source=replay_noise_source(53))
    src = replay_noise_source(53)
    want = _by_hand(lambda k: d.sample(2 * k, m, sar.repeat(k, 1, 1, 1), NDVI_channels=1, noise_source=src,
                                       sampling_steps=S_STEPS), [2, 2, 1], 2)
    assert got.shape == (5, 2, 1, SIZE, SIZE) and torch.equal(got, want) and not torch.equal(got[0], got[1])


def test_sample_ensemble_generation_is_three_sample_calls(dev, seeded_sd_gen):
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl("mfma_f32")
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T_STEPS, device=dev, image_size=32)
    cls = torch.tensor([2, 5])
    got = d.sample_ensemble(5, m, target_class=cls, cfg_scale=3, member_batch=2, sampling_steps=S_STEPS,
                            noise_source=replay_noise_source(54))
    src = replay_noise_source(54)
    want = _by_hand(lambda k: d.sample(2 * k, m, target_class=cls.repeat(k), cfg_scale=3, noise_source=src,
                                       sampling_steps=S_STEPS), [2, 2, 1], 2)
    assert got.shape == (5, 2, 3, 32, 32) and torch.equal(got, want) and not torch.equal(got[0], got[1])


# ---------------------------------------------------------------------------------------------
# Diffusion.evaluate(ensemble=N) and the command line
# ---------------------------------------------------------------------------------------------
def _recording(source):
    draws = []

    def src(i, shape):
        draws.append(source(i, shape))
        return draws[-1]
    return src, draws


def _replaying(draws):
    it = iter(draws)
    return lambda i, shape: next(it)


def _stack(per_image):
    return {k: torch.tensor(v, dtype=torch.float64) for k, v in per_image.items()}


def _assert_quality(got, want, what):
    """The tolerances of tests/test_gpu_metrics.py: PSNR 1e-3 dB, SSIM 1e-5, SAM 1e-4 degrees or relative, ERGAS 1e-5 relative."""
    assert set(got) == set(want), what
    for k, w in want.items():
        bound = {"psnr": 1e-3, "ssim": 1e-5, "sam": max(1e-4, 1e-4 * w.abs().max().item()), "ergas": 1e-5 * w.abs().max().item()}[k]
        assert (got[k] - w).abs().max().item() <= bound, (what, k)


def _check_evaluate(d, m, loader, truth, sample_members, mag, seed):
    """`evaluate(ensemble=3)` over two batches of two images, one member per sampling call so that member 0 of a batch is the
    draw plain `evaluate` makes: "member" is that figure, "model" scores the oracle mean of the members a direct
    `sample_ensemble` returns, "ensemble" the oracle's scores of those members."""
    src, draws = _recording(replay_noise_source(seed))
    res = d.evaluate(m, loader, sampling_steps=S_STEPS, noise_source=src, ensemble=3, member_batch=1)
    assert not m.training and res["n"] == 4 and len(draws) == 6  # eta = 0: one draw, x_T, per chunk
    plain = d.evaluate(m, loader, sampling_steps=S_STEPS, noise_source=_replaying([draws[0], draws[3]]))
    assert "member" not in plain and "ensemble" not in plain and "ensemble" not in plain["per_image"]
    assert set(res) == set(plain) | {"member", "ensemble"}
    assert res["member"] == plain["model"] and res["per_image"]["member"] == plain["per_image"]["model"]
    src = replay_noise_source(seed)
    members = []
    for cond, _ in loader:
        members.append(sample_members(cond, src).cpu())
        m.eval()
    members = torch.cat(members, dim=1)
    assert members.shape[:2] == (3, 4)
    mean = EO.statistics(members, (), (0.0, 1.0))["mean"]
    _assert_quality(_stack(res["per_image"]["model"]), MO.image_quality(mean, truth, mag), "mean")
    want = EO.scores(members, truth, (0.0, 1.0))
    got = res["per_image"]["ensemble"]
    assert set(got) == set(res["ensemble"]) == {"crps", "spread", "rmse", "spread_skill", "rank_histogram"}
    for k in ("crps", "spread", "rmse", "spread_skill"):
        _assert_sums(torch.tensor(got[k], dtype=torch.float64), want[k], k)
        assert res["ensemble"][k] == pytest.approx(want[k].mean().item(), rel=1e-11)
    assert got["rank_histogram"] == want["rank_histogram"].tolist()
    assert res["ensemble"]["rank_histogram"] == want["rank_histogram"].sum(dim=0).tolist()
    assert sum(res["ensemble"]["rank_histogram"]) == truth.numel()
    # all members in one sampling call: same keys, finite figures
    whole = d.evaluate(m, loader, n_images=3, sampling_steps=S_STEPS, noise_source=replay_noise_source(seed), ensemble=3)
    assert whole["n"] == 3 and len(whole["per_image"]["ensemble"]["crps"]) == 3
    assert all(math.isfinite(whole["ensemble"][k]) for k in ("crps", "spread", "rmse", "spread_skill"))


def test_evaluate_ensemble_superres(dev, seeded_sd):
    from diffusionremotesensing_amd import synthetic
    m, d = _superres(dev, seeded_sd)
    hr = synthetic.tensor_uniform("metrics.hr", (4, 3, SIZE, SIZE))
    lr = synthetic.tensor_uniform("metrics.lr", (4, 3, SIZE // MAG, SIZE // MAG))
    loader = [(lr[:2], hr[:2]), (lr[2:], hr[2:])]
    _check_evaluate(d, m, loader, hr, lambda cond, src: d.sample_ensemble(
        3, m, cond.to(dev), input_channels=3, member_batch=1, sampling_steps=S_STEPS, noise_source=src), MAG, 61)
    with pytest.raises(ValueError, match="known_mask_fn"):
        d.evaluate(m, loader, ensemble=3, known_mask_fn=lambda t: t)


def test_evaluate_ensemble_sar_to_ndvi(dev, seeded_sd_sar):
    from diffusionremotesensing_amd import synthetic
    m, d = _sar(dev, seeded_sd_sar)
    sar = synthetic.tensor_uniform("metrics.sar", (4, 2, SIZE, SIZE))
    ndvi = synthetic.tensor_uniform("metrics.ndvi", (4, 1, SIZE, SIZE))
    loader = [(sar[:2], ndvi[:2]), (sar[2:], ndvi[2:])]
    _check_evaluate(d, m, loader, ndvi, lambda cond, src: d.sample_ensemble(
        3, m, cond.to(dev), NDVI_channels=1, member_batch=1, sampling_steps=S_STEPS, noise_source=src), None, 62)


_TRAIN = ["--epochs", "1", "--batch_size", "4", "--image_size", "32", "--noise_steps", "10", "--loss", "MSE",
          "--magnification_factor", "2", "--dataset_path", "synthetic:8", "--check_preds_epoch", "1", "--sampling_steps", "3"]


def test_evaluate_command_with_and_without_the_flag(dev, tmp_path, monkeypatch, capsys):
    """`evaluate.main --ensemble 3` on a one-epoch snapshot prints the `member` row and the ensemble line and writes the
    documented JSON keys with finite values; without the flag it writes exactly the keys it wrote before."""
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    T.main(_TRAIN + ["--model_name", "cli_ensemble"])
    capsys.readouterr()
    common = ["--model_name", "cli_ensemble", "--image_size", "32", "--noise_steps", "10", "--batch_size", "4",
              "--magnification_factor", "2", "--dataset_path", "synthetic:4", "--sampling_steps", "3"]
    evaluate.main(common + ["--ensemble", "3", "--member_batch", "2", "--out", str(tmp_path / "e.json")])
    out = capsys.readouterr().out
    rows = [ln.split()[0] for ln in out.splitlines() if ln.split()]
    assert "model" in rows and "member" in rows and "bicubic" in rows and "ensemble" in rows
    assert "CRPS" in out and "spread/skill" in out and "rank histogram" in out and "ensembles of 3 members" in out
    saved = json.load(open(tmp_path / "e.json"))
    assert set(saved) == {"model", "member", "bicubic", "ensemble", "per_image", "n", "args"}
    assert set(saved["per_image"]) == {"model", "member", "bicubic", "ensemble"}
    for name in ("model", "member", "bicubic"):
        assert set(saved[name]) == {"psnr", "ssim", "sam", "ergas"}
        assert all(math.isfinite(v) for v in saved[name].values()), saved[name]
    assert set(saved["ensemble"]) == {"crps", "spread", "rmse", "spread_skill", "rank_histogram"}
    assert all(math.isfinite(saved["ensemble"][k]) for k in ("crps", "spread", "rmse", "spread_skill"))
    assert len(saved["ensemble"]["rank_histogram"]) == 4 and sum(saved["ensemble"]["rank_histogram"]) == saved["n"] * 3 * 32 * 32
    evaluate.main(common + ["--out", str(tmp_path / "p.json")])
    out = capsys.readouterr().out
    assert "member" not in out and "CRPS" not in out
    plain = json.load(open(tmp_path / "p.json"))
    assert set(plain) == {"model", "bicubic", "per_image", "n", "args"} and set(plain["per_image"]) == {"model", "bicubic"}
