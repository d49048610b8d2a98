"""The entry points of csrc/terminal_step.hip between guard bands at the three pointer phases of tests/guard.py, run through
`test_gpu_guard.guarded_runs` - so that they count for that module's `test_every_entry_point_that_launches_is_guarded`, which
walks `_lib.SIGNATURES` and runs after this file (files run in name order; on its own that test does not know these entries)."""
import pytest
import torch

import test_gpu_guard as G
import ztsnr_oracle as Z

pytestmark = pytest.mark.gpu

T50 = 50


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("mask_channels", [1, 3])
def test_terminal_step_between_guards(monkeypatch, dev, mask_channels):
    """Guided v prediction, threshold scales, noise, known pixels and the history on (2, 3, 5, 7) (chw = 105: head, groups and
    tail): aligned, every tensor one float into its line (the 16-byte path at phase 1), and mixed (element by element) give the
    bits of the normal call, inside the float64 oracle's bound, with every guard intact."""
    from diffusionremotesensing_amd import hip_ops
    shape = (2, 3, 5, 7)
    g = torch.Generator().manual_seed(9)
    x, z, pred = (torch.randn(shape, generator=g) for _ in range(3))
    pu = pred * (1 + 0.1 * (2 * torch.rand(shape, generator=g) - 1))
    known = torch.rand(shape, generator=g)
    mask = (torch.rand((2, mask_channels, 5, 7), generator=g) < 0.4).to(torch.uint8)
    scale, clip = torch.tensor([0.3, 1.7]), (-1.0, 1.0)
    ah = Z.schedule("cosine", T50)[1]

    def fn(put):
        xs, hist = put(x.to(dev)), put(torch.zeros(shape).to(dev))
        hip_ops.terminal_step_(xs, put(pred.to(dev)), put(z.to(dev)), T50 - 1, 23, put(ah.to(dev)), "v", eta=0.5, x0_clip=clip,
                               scale=put(scale.to(dev)), pred_uncond=put(pu.to(dev)), cfg_scale=3.0, known=put(known.to(dev)),
                               known_mask=put(mask.to(dev)), hist=hist)
        return {"x": xs, "x0_hist": hist}

    def oracle(res):
        want, x0, terms = Z.terminal_step(x, pred, z, 23, ah, "v", 0.5, clip, scale, pu, 3.0, known, mask)
        unknown = (mask == 0).expand(shape)
        bound = 2.0 ** -22 * terms + 2.0 ** -23 * x0.abs()
        assert bool(((res["x"].cpu().double() - want).abs() <= bound)[unknown].all())
    G.guarded_runs(monkeypatch, dev, "drs_terminal_step", fn, oracle, case=f"mask of {mask_channels}")


@pytest.mark.parametrize("chw", [105, 4097])
def test_cfg_rescale_between_guards(monkeypatch, dev, chw):
    """n = 3; the workspace is allocated inside the block (the cache is emptied before every run), so it is guarded too."""
    from diffusionremotesensing_amd import hip_ops
    g = torch.Generator().manual_seed(chw)
    cond, uncond = torch.randn((3, chw), generator=g) * 0.7 + 0.2, torch.randn((3, chw), generator=g)

    def fn(put):
        out = put(torch.zeros((3, chw)).to(dev))
        hip_ops.cfg_rescale(put(cond.to(dev)), put(uncond.to(dev)), 3.0, 0.7, out=out)
        return {"out": out}

    def oracle(res):
        want, _ = Z.cfg_rescale(cond, uncond, 3.0, 0.7)
        assert bool(((res["out"].cpu().double() - want).abs() <= 3 * 2.0 ** -24 * want.abs()).all())
    G.guarded_runs(monkeypatch, dev, "drs_cfg_rescale", fn, oracle, setup=hip_ops._RESCALE_WS.clear, case=f"chw {chw}")
