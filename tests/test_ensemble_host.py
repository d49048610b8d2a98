"""Ensemble statistics without a GPU: the float64 oracle against brute force and numpy, the argument validation of the new
C-ABI entry points, the chunking of `sample_ensemble` on a stub sampler, and the command line's parser errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import ensemble_oracle as EO

MEMBER_COUNTS = [2, 3, 5, 8, 17, 32]


def _case(N, seed, shape=(2, 3, 5, 7)):
    """Members quantised to steps of 0.25 (ties among members) and a truth that equals a member at every third element."""
    g = torch.Generator().manual_seed(100 * N + seed)
    x = torch.round(torch.randn((N,) + shape, generator=g, dtype=torch.float64) * 4) / 4 + 0.0
    y = torch.randn(shape, generator=g, dtype=torch.float64)
    pick = torch.randint(0, N, shape, generator=g)
    hit = (torch.arange(y.numel()).view(shape) % 3) == 0
    return x, torch.where(hit, torch.gather(x, 0, pick[None])[0], y)


@pytest.mark.parametrize("N", MEMBER_COUNTS)
def test_oracle_crps_sorted_form_equals_pairwise_form(N):
    for seed, smooth in ((0, False), (1, True)):
        x, y = _case(N, seed)
        if smooth:
            x = x + 0.1 * torch.randn(x.shape, generator=torch.Generator().manual_seed(N), dtype=torch.float64)
        else:
            s = torch.sort(x, dim=0).values
            assert (s[1:] == s[:-1]).any() and (x == y).any()  # ties among members and with the truth occur
        assert (EO.crps_map(x, y) - EO.crps_pairwise(x, y)).abs().max().item() <= 1e-13


@pytest.mark.parametrize("N", MEMBER_COUNTS)
def test_oracle_statistics_against_numpy(N):
    x, _ = _case(N, 2)
    qs = (0.0, 0.05, 1 / 3, 0.5, 0.95, 1.0)
    st = EO.statistics(x, qs)
    a = x.numpy()
    assert np.abs(st["quantiles"].numpy() - np.quantile(a, qs, axis=0)).max() <= 1e-13
    assert np.abs(st["mean"].numpy() - a.mean(axis=0)).max() <= 1e-13
    assert np.abs(st["std"].numpy() - a.std(axis=0, ddof=1)).max() <= 1e-13
    assert torch.equal(st["quantiles"][0], x.amin(dim=0)) and torch.equal(st["quantiles"][-1], x.amax(dim=0))


def test_oracle_ranks_nan_and_clamp():
    x = torch.tensor([0.5, -1.0, 2.0, 0.5]).view(4, 1, 1, 1, 1)
    y = torch.tensor([0.5]).view(1, 1, 1, 1)
    assert EO.ranks(x, y)[0].item() == 1  # a member equal to the truth is not below it
    assert EO.ranks(x, y, clamp=(0.0, 1.0))[0].item() == 1 and EO.statistics(x, clamp=(0.0, 1.0))["mean"].item() == 0.5
    assert EO.rank_histogram(x, y).tolist() == [[0, 1, 0, 0, 0]]
    x[2] = float("nan")
    assert torch.isnan(EO.statistics(x, (0.5,))["quantiles"]).all() and torch.isnan(EO.sums(x, y)).all()
    assert EO.rank_histogram(x, y).sum().item() == 0
    cal = EO.scores(torch.randn((8, 1, 1, 64, 64), generator=torch.Generator().manual_seed(5)),
                    torch.randn((1, 1, 64, 64), generator=torch.Generator().manual_seed(6)))
    assert abs(cal["spread_skill"].item() - 1.0) < 0.05  # truth drawn from the members' distribution: calibrated


def test_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(1 << 16)
    p = C.cast(buf, C.c_void_p)
    q = (C.c_double * 9)(0.0, 0.5, 1.0, 0.1, 0.2, 0.3, 0.4, 0.6, 0.7)
    qp = C.cast(q, C.c_void_p)

    def stats(members=p, mean=p, quant=p, qv=qp, Q=3, N=4):
        return lib.drs_ensemble_stats(members, mean, p, quant, qv, Q, N, 1, 3, 8, 8, 0, 0.0, 0.0, None)

    def scores(ptrs=(p, p, p, p, p), N=4, ws=p, ws_bytes=1 << 16):
        return lib.drs_ensemble_scores(*ptrs, N, 1, 3, 8, 8, 1, 0.0, 1.0, ws, ws_bytes, None)
    assert stats(members=None) == 1 and b"null pointer" in lib.drs_last_error()
    assert stats(quant=None) == 1 and b"null pointer" in lib.drs_last_error()
    assert stats(qv=None) == 1 and b"null pointer" in lib.drs_last_error()
    for n in (1, 33, 0, -2):
        assert stats(N=n) == 2 and b"members" in lib.drs_last_error()
        assert scores(N=n) == 2 and b"members" in lib.drs_last_error()
    assert stats(Q=9) == 2 and b"quantiles" in lib.drs_last_error()
    q[1] = 1.5
    assert stats() == 2 and b"outside [0, 1]" in lib.drs_last_error()
    q[1] = -0.25
    assert stats() == 2
    q[1] = float("nan")
    assert stats() == 2
    for hole in (0, 1, 3, 4):  # members, truth, sums, rank histogram (the CRPS map is optional)
        assert scores(tuple(None if i == hole else p for i in range(5))) == 1
        assert b"null pointer" in lib.drs_last_error()
    assert scores(ws=None) == 1
    assert scores(ws_bytes=8) == 4
    assert lib.drs_ensemble_scores(p, p, p, p, p, 4, 0, 3, 8, 8, 0, 0.0, 0.0, p, 1 << 16, None) == 2
    sizes = [lib.drs_ensemble_workspace_bytes(8, b, 3, 40, 52) for b in (1, 2, 3, 16)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == 4  # monotone in B
    assert lib.drs_ensemble_workspace_bytes(1, 2, 3, 8, 8) == 0 and lib.drs_ensemble_workspace_bytes(33, 2, 3, 8, 8) == 0


def test_wrappers_have_no_cpu_path():
    from diffusionremotesensing_amd import ensemble_scores, ensemble_statistics, hip_ops
    x, y = torch.rand(4, 1, 3, 8, 8), torch.rand(1, 3, 8, 8)
    for call in (lambda: ensemble_statistics(x), lambda: ensemble_scores(x, y), lambda: hip_ops.ensemble_stats(x),
                 lambda: hip_ops.ensemble_scores(x, y), lambda: ensemble_scores(x[:, 0], y[0])):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


class _Recorder:
    """Stands in for `sample` / `sample_known`: records the call, asks the noise source once for x_T and returns it."""

    def __init__(self):
        self.calls = []

    def sample(self, n, model, cond=None, **kw):
        self.calls.append(("sample", n, None if cond is None else tuple(cond.shape), kw.get("target_class")))
        return kw["noise_source"](8, (n, 3, 4, 4))

    def sample_known(self, n, model, *rest, **kw):
        self.calls.append(("sample_known", n, tuple(tuple(t.shape) for t in rest if t is not None), kw["resample"]))
        return kw["noise_source"](8, (n, 3, 4, 4))


def _stub(cls):
    rec = _Recorder()
    d = object.__new__(cls)
    d.sample, d.sample_known = rec.sample, rec.sample_known
    return d, rec


def _counting_source():
    asked = []

    def src(i, shape):
        asked.append((i, tuple(shape)))
        return torch.full(shape, float(len(asked)))
    return src, asked


def test_sample_ensemble_chunks_and_noise_order():
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion, ensemble_chunks
    assert ensemble_chunks(5, 2) == [2, 2, 1] and ensemble_chunks(5) == [5] and ensemble_chunks(4, 9) == [4]
    assert ensemble_chunks(6, 3) == [3, 3] and ensemble_chunks(3, 1) == [1, 1, 1]
    d, rec = _stub(Diffusion)
    src, asked = _counting_source()
    lr = torch.arange(3 * 3 * 2 * 2, dtype=torch.float32).view(3, 3, 2, 2)
    out = d.sample_ensemble(5, "model", lr, member_batch=2, sampling_steps=4, noise_source=src)
    assert out.shape == (5, 3, 3, 4, 4)
    assert [c[:3] for c in rec.calls] == [("sample", 6, (6, 3, 2, 2)), ("sample", 6, (6, 3, 2, 2)), ("sample", 3, (3, 3, 2, 2))]
    assert asked == [(8, (6, 3, 4, 4)), (8, (6, 3, 4, 4)), (8, (3, 3, 4, 4))]  # chunk after chunk
    assert [out[m, 0, 0, 0, 0].item() for m in range(5)] == [1, 1, 2, 2, 3]  # member-major
    one = d.sample_ensemble(2, "model", lr[0], noise_source=src)  # a single image: B = 1, all members at once
    assert one.shape == (2, 1, 3, 4, 4) and rec.calls[-1][:3] == ("sample", 2, (2, 3, 2, 2))
    known, mask = torch.zeros(3, 3, 4, 4), torch.ones(4, 4)
    d.sample_ensemble(3, "model", lr, member_batch=2, noise_source=src, known=known, known_mask=mask, resample=2)
    assert rec.calls[-2:] == [("sample_known", 6, ((6, 3, 2, 2), (6, 3, 4, 4), (4, 4)), 2),
                              ("sample_known", 3, ((3, 3, 2, 2), (3, 3, 4, 4), (4, 4)), 2)]


def test_sample_ensemble_of_the_other_two_models():
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as Gen
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as Sar
    d, rec = _stub(Sar)
    src, asked = _counting_source()
    out = d.sample_ensemble(5, "model", torch.zeros(2, 2, 4, 4), NDVI_channels=3, member_batch=2, noise_source=src)
    assert out.shape == (5, 2, 3, 4, 4) and [c[1] for c in rec.calls] == [4, 4, 2] and len(asked) == 3
    d, rec = _stub(Gen)
    out = d.sample_ensemble(5, "model", torch.tensor([3, 7]), cfg_scale=3, member_batch=2, noise_source=src)
    assert out.shape == (5, 2, 3, 4, 4)
    assert [c[3].tolist() for c in rec.calls] == [[3, 7, 3, 7], [3, 7, 3, 7], [3, 7]]
    assert d.sample_ensemble(2, "model", None, noise_source=src).shape == (2, 1, 3, 4, 4) and rec.calls[-1][3] is None


@pytest.mark.parametrize("n_members,member_batch", [(1, None), (0, None), (2.5, None), (True, None), (4, 0), (4, 1.5), (4, -1)])
def test_sample_ensemble_argument_errors(n_members, member_batch):
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion as Gen
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion as Sar
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    for cls, cond in ((Diffusion, torch.zeros(2, 3, 2, 2)), (Sar, torch.zeros(2, 2, 4, 4)), (Gen, torch.tensor([1, 2]))):
        d, rec = _stub(cls)
        with pytest.raises(ValueError, match="n_members|member_batch"):
            d.sample_ensemble(n_members, "model", cond, member_batch=member_batch)
        assert rec.calls == []  # nothing was sampled
    d, rec = _stub(Diffusion)
    with pytest.raises(ValueError):
        d.evaluate("model", [], ensemble=1)
    with pytest.raises(ValueError, match="member_batch"):
        d.evaluate("model", [], member_batch=2)


def test_evaluate_parser_errors_and_formats(capsys):
    from diffusionremotesensing_amd import evaluate
    base = ["--model_name", "m", "--image_size", "64", "--magnification_factor", "2"]
    for bad in (["--ensemble", "1"], ["--ensemble", "33"], ["--member_batch", "2"], ["--ensemble", "4", "--member_batch", "0"],
                ["--ensemble", "4", "--known_fraction", "0.5"]):
        with pytest.raises(SystemExit):
            evaluate.main(base + bad)
        assert "--ensemble" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate.main(base + ["--task", "sar_to_ndvi", "--member_batch", "2"])
    p = evaluate.add_ensemble_args(evaluate.evaluate_arg_parser())
    a = p.parse_args(base + ["--ensemble", "8", "--member_batch", "4"])
    assert (a.ensemble, a.member_batch) == (8, 4)
    d = p.parse_args(base)
    assert d.ensemble is None and d.member_batch is None
    scores = {"model": {"psnr": 24.0, "ssim": 0.9}, "member": {"psnr": 22.0, "ssim": 0.8}, "bicubic": {"psnr": 20.0, "ssim": 0.5},
              "ensemble": {"crps": 0.01234567, "spread": 0.02, "rmse": 0.025, "spread_skill": 0.9237, "rank_histogram": [3, 1, 2]}}
    rows = [ln.split()[0] for ln in evaluate.format_table(scores).splitlines()[1:]]
    assert rows == ["model", "member", "bicubic"]
    assert evaluate.format_ensemble(scores["ensemble"]) == ("ensemble  CRPS 0.01235  spread 0.02  RMSE 0.025  "
                                                            "spread/skill 0.924  rank histogram [3, 1, 2]")
