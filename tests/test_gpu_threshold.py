"""Dynamic x0 thresholding on the GPU: the radix select of drs_x0_quantile against a CPU sort, bit for bit;
drs_pred_to_eps_dyn against the float64 oracle of tests/threshold_oracle.py; its bit identities with the static clip; and
`Diffusion(x0_clip=, x0_threshold=)` chains of the samplers and the tiler against the existing float64 chains fed the oracle's
thresholded eps."""
import math
import types

import numpy as np
import pytest
import torch

import prediction_oracle as PO
import threshold_oracle as TO
import tile_chain_oracle as TC
from conftest import rel_errors, replay_noise_source
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U

pytestmark = pytest.mark.gpu

IMPL = "mfma_bf16x3"
KERNEL_BAR = 1e-6  # the project's bar for its step kernels: error / largest sum of |terms|
SCALE_BAR = 1e-6   # the scales, relative to the oracle's
SCHEDULES = {"cosine": 1500, "linear": 1000}
# one sweep of the capped grid is 2048 blocks x 256 threads x 4 elements: the last shape takes a second one, and a scalar tail
LONG = (1, 1, 1, 2048 * 256 * 4 + 1029)
SHAPES = [(1, 1, 1, 1), (3, 1, 5, 7), (2, 3, 16, 20), (2, 1, 1, 4097), LONG]
CLIPS = ((0.0, 1.0), (-1.0, 1.0))
GUIDES = (None, 0.3, 3.0)
QUANTILES = (1e-9, 0.5, 0.995, 1.0)
INF_KEY = 0x7f800000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table(dev):
    _, ah, _ = D.schedule("cosine", 50)
    return ah, ah.to(dev)


def _ids(shape):
    return "x".join(map(str, shape))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------
# the selection, bit for bit
# ---------------------------------------------------------------------------------------------
def _want_scales(pred, clip, p):
    """sort(|fl(pred - c)|)[k] per image in fp32 on the CPU: for an x0 network d is one exact-rounded fp32 subtraction."""
    c, _ = TO.centre_and_half_range(clip)
    dev_abs = (pred.flatten(1) - torch.tensor(c, dtype=torch.float32)).abs()
    assert dev_abs.dtype == torch.float32 and torch.isfinite(dev_abs).all()
    return dev_abs.sort(dim=1).values[:, TO.rank_of(p, dev_abs.shape[1])]


def _select(dev, table, pred, clip, p):
    from diffusionremotesensing_amd import hip_ops
    n = pred.shape[0]
    x = torch.zeros_like(pred).to(dev)
    t = torch.full((n,), 7, dtype=torch.int64, device=dev)
    return hip_ops.x0_abs_quantile(pred.to(dev), x, t, table[1], "x0", clip, p).cpu()


def _check_select(dev, table, pred, clip, ps, what):
    for p in ps:
        got, want = _select(dev, table, pred, clip, p), _want_scales(pred, clip, p)
        assert got.dtype == torch.float32 and torch.equal(_bits(got), _bits(want)), (what, clip, p, got, want)


def _patterns(chw, stride, seed):
    """chw floats from the bit patterns base + i stride (all below +inf's; the top digit has 2040 values, so i wraps there),
    randomly permuted and randomly signed."""
    rng = np.random.default_rng(seed)
    distinct = min(chw, (INF_KEY - (1 << 20)) // stride)
    # low digit: anywhere; middle digit: from 0x3e8..... (0.25) up, d = value - 0.5 is exact there; top digit: from the denormals up
    base = {1: int(rng.integers(1 << 20, 1 << 30)), 1 << 10: 0x3e800000 + int(rng.integers(0, 1 << 10)),
            1 << 20: int(rng.integers(1, 1 << 20))}[stride]
    bits = base + (np.arange(chw, dtype=np.int64) % distinct) * stride
    assert bits.max() < INF_KEY
    bits = rng.permutation(bits) | (rng.integers(0, 2, chw, dtype=np.int64) << 31)
    return torch.from_numpy(bits.astype(np.uint32).view(np.float32).copy())


@pytest.mark.parametrize("clip", CLIPS, ids=["clip01", "clip11"])
@pytest.mark.parametrize("stride", [1, 1 << 10, 1 << 20], ids=["low", "middle", "top"])
def test_select_one_digit_at_a_time(dev, table, clip, stride):
    """Keys that differ in one digit only: the low, the middle or the top one decides the rank."""
    for chw in (1900, 2048, 4099):
        pred = torch.stack([_patterns(chw, stride, 10 * chw + i) for i in range(3)]).view(3, 1, 1, chw)
        _check_select(dev, table, pred, clip, QUANTILES + (0.25, 0.75), ("patterns", chw, stride))


@pytest.mark.parametrize("clip", CLIPS, ids=["clip01", "clip11"])
@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_select_ties_and_small_values(dev, table, clip, shape):
    g = torch.Generator().manual_seed(31)
    n, chw = shape[0], math.prod(shape[1:])
    c, _ = TO.centre_and_half_range(clip)
    equal = torch.full(shape, 0.8125)
    zeros = torch.zeros(shape) + c  # d = +0 and -0 mixed
    zeros = torch.where(torch.rand(shape, generator=g) < 0.5, zeros, -zeros if c == 0 else zeros)
    denormal = torch.from_numpy(np.random.default_rng(7).integers(1, 1 << 23, n * chw, dtype=np.int64).astype(np.uint32)
                                .view(np.float32).copy()).view(shape)
    denormal = denormal * torch.where(torch.rand(shape, generator=g) < 0.5, 1.0, -1.0)
    grid = torch.randint(0, 256, shape, generator=g).float() / 255.0 * 1.4 - 0.2
    mixed = torch.randn(shape, generator=g)
    for what, pred in (("equal", equal), ("zeros", zeros), ("denormal", denormal), ("grid", grid), ("randn", mixed)):
        _check_select(dev, table, pred, clip, QUANTILES, (what, shape))
    if c == 0:
        assert (_bits(zeros) != 0).any() or chw < 4  # -0.0 is among them
        assert (_select(dev, table, zeros, clip, 1.0) == 0).all() and (_bits(_select(dev, table, zeros, clip, 1.0)) == 0).all()
    # two distinct values, k on the last of the low group and on the first of the high group
    if chw >= 2:
        low_count = max(1, chw // 3)
        two = torch.full((n, chw), c + 1.75)
        two[:, :low_count] = c + 0.25
        two = two[:, torch.randperm(chw, generator=g)].view(shape)
        for k, want in ((low_count - 1, 0.25), (low_count, 1.75)):
            got = _select(dev, table, two, clip, (k + 0.5) / (chw - 1))
            assert torch.equal(got, torch.full((n,), want)), (shape, k, got)


def test_select_long_image(dev, table):
    """A second grid sweep and a scalar tail, once."""
    g = torch.Generator().manual_seed(32)
    pred = torch.randn(LONG, generator=g)
    _check_select(dev, table, pred, (0.0, 1.0), (0.5, 0.995), "long")
    _check_select(dev, table, pred, (-1.0, 1.0), (1e-9, 1.0), "long")


# ---------------------------------------------------------------------------------------------
# the kernel against the float64 oracle
# ---------------------------------------------------------------------------------------------
def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(shape, generator=g) for _ in range(3)]


def _norm_err(got, want, bound):
    top = bound.max().item()
    err = (got.double() - want).abs().max().item()
    return err / top if top > 0 else err


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", list(SCHEDULES))
def test_threshold_kernel_vs_float64_oracle(dev, kind, shape):
    """The grid of test_pred_to_eps_kernel_vs_float64_oracle - levels {1, 7, T/2, T-1} mixed within the batch, every prediction x
    clip x guidance - at p in {0.5, 0.995, 1.0}: error / max(sum of |terms|) <= 1e-6, scales within 1e-6 relative.  The long
    image takes every prediction and clip at T/2, unguided, p = 0.995, and one guided case."""
    from diffusionremotesensing_amd import hip_ops
    T = SCHEDULES[kind]
    _, ah, _ = D.schedule(kind, T)
    ah_d = ah.to(dev)
    x, pc, pu = _inputs(shape, 41)
    xd, pcd, pud = x.to(dev), pc.to(dev), pu.to(dev)
    n, lv, long = shape[0], [1, 7, T // 2, T - 1], shape == LONG
    rotations = [[lv[2]] * n] if long else [[lv[(i + r) % 4] for i in range(n)] for r in range(4)]
    worst, worst_scale = 0.0, 0.0
    for levels in rotations:
        t = torch.tensor(levels)
        td = t.to(dev)
        for pk in PO.KINDS:
            for clip in CLIPS:
                for w in GUIDES:
                    for p in (0.5, 0.995, 1.0):
                        if long and (p != 0.995 or (w is not None and (w, pk, clip) != (3.0, "v", (0.0, 1.0)))):
                            continue
                        p64 = pc.double() if w is None else pu.double() + w * (pc.double() - pu.double())
                        want, bound, want_s = TO.to_eps(pk, p64, x, ah, t, clip, p)
                        guided = {"pred_uncond": pud, "cfg_scale": w} if w is not None else {}
                        scales = torch.empty(n, device=dev)
                        got = hip_ops.pred_to_eps_(pcd, xd, td, ah_d, pk, clip, out=torch.empty_like(pcd), x0_threshold=p,
                                                   scale_out=scales, **guided)
                        err = _norm_err(got.cpu(), want, bound)
                        err_s = ((scales.cpu().double() - want_s).abs() / want_s.abs().clamp_min(1e-300)).max().item()
                        worst, worst_scale = max(worst, err), max(worst_scale, err_s)
                        if err > KERNEL_BAR or err_s > SCALE_BAR:
                            print(f"threshold kernel MISS [{kind} {shape}] {levels} {pk} {clip} w={w} p={p}: {err:.3e} {err_s:.3e}")
                        assert err <= KERNEL_BAR and err_s <= SCALE_BAR, (kind, shape, levels, pk, clip, w, p, err, err_s)
    print(f"threshold kernel [{kind} {shape}]: worst normalised error {worst:.3e}, worst relative scale error {worst_scale:.3e}")


# ---------------------------------------------------------------------------------------------
# bit identities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[1:4], ids=_ids)
@pytest.mark.parametrize("pk", PO.KINDS)
def test_calls_repeat_and_in_place_is_out(dev, pk, shape):
    from diffusionremotesensing_amd import hip_ops
    T = 1500
    _, ah, _ = D.schedule("cosine", T)
    ah_d = ah.to(dev)
    x, pc, pu = (a.to(dev) for a in _inputs(shape, 42))
    t = torch.tensor([7, T // 2, T - 1][:shape[0]]).to(dev)
    for clip in CLIPS:
        for guided in ({}, {"pred_uncond": pu, "cfg_scale": 3.0}):
            for p in (0.5, 0.995):
                s1, s2 = torch.empty(shape[0], device=dev), torch.empty(shape[0], device=dev)
                out = torch.empty_like(pc)
                got = hip_ops.pred_to_eps_(pc, x, t, ah_d, pk, clip, out=out, x0_threshold=p, scale_out=s1, **guided)
                again = hip_ops.pred_to_eps_(pc, x, t, ah_d, pk, clip, out=torch.empty_like(pc), x0_threshold=p, scale_out=s2,
                                             **guided)
                inplace = hip_ops.pred_to_eps_(pc.clone(), x, t, ah_d, pk, clip, x0_threshold=p, **guided)
                assert got is out and torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(got), _bits(inplace))
                alone = hip_ops.x0_abs_quantile(pc, x, t, ah_d, pk, clip, p, **guided)
                assert torch.equal(_bits(s1), _bits(s2)) and torch.equal(_bits(s1), _bits(alone))
    # a view that starts elsewhere in its 16-byte line than the state: element by element, the same values
    buf = torch.empty(pc.numel() + 1, device=dev)
    shifted = buf[1:].view(shape)
    shifted.copy_(pc)
    assert torch.equal(hip_ops.pred_to_eps_(shifted, x, t, ah_d, pk, (0.0, 1.0), x0_threshold=0.995),
                       hip_ops.pred_to_eps_(pc.clone(), x, t, ah_d, pk, (0.0, 1.0), x0_threshold=0.995))


@pytest.mark.parametrize("clip", CLIPS, ids=["clip01", "clip11"])
@pytest.mark.parametrize("pk", PO.KINDS)
def test_a_scale_inside_the_range_is_the_static_clip(dev, pk, clip):
    """One batch with both kinds of image: images whose scale is <= r carry the bits of `pred_to_eps_(..., x0_clip)`, the
    others do not; the x0 every returned eps implies lies in [lo, hi] up to the kernel bar."""
    from diffusionremotesensing_amd import hip_ops
    T, shape = 1500, (4, 3, 16, 20)
    _, ah, _ = D.schedule("cosine", T)
    ah_d = ah.to(dev)
    c, r = TO.centre_and_half_range(clip)
    g = torch.Generator().manual_seed(43)
    t = torch.tensor([7, 7, T // 2, T // 2])
    x = torch.randn(shape, generator=g)
    x0 = c + r * torch.randn(shape, generator=g) * torch.tensor([0.3, 3.0, 0.3, 3.0]).view(4, 1, 1, 1)  # narrow | wide
    pred = PO.from_eps(pk, (x.double() - PO.a_s(ah, t)[0] * x0.double()) / PO.a_s(ah, t)[1], x, ah, t).float()
    scales = torch.empty(4, device=dev)
    got = hip_ops.pred_to_eps_(pred.to(dev), x.to(dev), t.to(dev), ah_d, pk, clip, out=torch.empty(shape, device=dev),
                               x0_threshold=0.9, scale_out=scales).cpu()
    static = hip_ops.pred_to_eps_(pred.to(dev), x.to(dev), t.to(dev), ah_d, pk, clip, out=torch.empty(shape, device=dev)).cpu()
    inside = (scales.cpu() <= r).tolist()
    assert inside == [True, False, True, False], scales
    for i in range(4):
        assert torch.equal(_bits(got[i]), _bits(static[i])) == inside[i], i
    a, s = PO.a_s(ah, t)
    implied = (x.double() - s * got.double()) / a
    terms = (x.double() / a).abs() + (s * got.double() / a).abs()
    lo, hi = clip
    assert ((implied - implied.clamp(lo, hi)).abs() <= KERNEL_BAR * terms.amax(dim=(1, 2, 3), keepdim=True)).all()
    # the thresholded images are compressed, not cut off: fewer elements sit on the range's edge than after the clamp
    x0_static = (x.double() - s * static.double()) / a
    for i in (1, 3):
        at_edge = lambda v: ((v - lo).abs() < 1e-4).sum() + ((v - hi).abs() < 1e-4).sum()  # noqa: E731
        assert at_edge(implied[i]) < at_edge(x0_static[i])


def test_degenerate_levels_are_pred_to_eps(dev):
    """Level 0 of the cosine table (alpha_hat = 1: ZERO), a t outside the table (BAD) and an eps network where alpha_hat = 0
    (PASS): those images are `pred_to_eps_`'s, bit for bit, their scale is 0, and their neighbours are thresholded as alone."""
    from diffusionremotesensing_amd import hip_ops
    T, shape = 1500, (4, 3, 16, 20)
    _, ah, _ = D.schedule("cosine", T)
    assert ah[0] == 1.0
    ah = ah.clone()
    ah[9] = 0.0
    ah_d = ah.to(dev)
    x, pc, pu = (a.to(dev) * 2 for a in _inputs(shape, 44))
    t = torch.tensor([0, 700, T + 3, 9]).to(dev)
    for pk in PO.KINDS:
        for guided in ({}, {"pred_uncond": pu, "cfg_scale": 3.0}):
            scales = torch.full((4,), -1.0, device=dev)
            got = hip_ops.pred_to_eps_(pc, x, t, ah_d, pk, (0.0, 1.0), out=torch.empty_like(pc), x0_threshold=0.9,
                                       scale_out=scales, **guided)
            static = hip_ops.pred_to_eps_(pc, x, t, ah_d, pk, (0.0, 1.0), out=torch.empty_like(pc), **guided)
            same = [0, 2] + ([3] if pk == "eps" else [])
            for i in same:
                assert torch.equal(_bits(got[i]), _bits(static[i])) and scales[i].item() == 0.0, (pk, i)
            assert (got[0] == 0).all() and torch.isnan(got[2]).all()
            one = {"pred_uncond": pu[1:2], "cfg_scale": 3.0} if guided else {}
            alone = hip_ops.pred_to_eps_(pc[1:2].clone(), x[1:2], t[1:2], ah_d, pk, (0.0, 1.0), x0_threshold=0.9, **one)
            assert torch.equal(_bits(got[1]), _bits(alone[0])) and scales[1].item() > 0.5
            assert not torch.equal(got[1], static[1])
    torch.cuda.synchronize()


@pytest.mark.parametrize("pk", PO.KINDS)
def test_planted_non_finite_values(dev, pk):
    """Fewer non-finite elements than the quantile leaves above it: the finite ones come out as if the others were +inf-ranked
    values, which stay non-finite.  More: the scale is +inf and the image is the static clip's."""
    from diffusionremotesensing_amd import hip_ops
    T, shape, clip, p = 1500, (2, 3, 16, 20), (0.0, 1.0), 0.9
    _, ah, _ = D.schedule("cosine", T)
    ah_d = ah.to(dev)
    x, pc, _ = _inputs(shape, 45)
    pc = pc * 2
    t = torch.tensor([7, T // 2])
    chw = 960
    few, many = [3, 100, 500, 959], list(range(0, 960, 8))  # 4 and 120 of 960: rank k = 863, so 96 lie above it
    for spots, inf_scale in ((few, False), (many, True)):
        bad = pc.clone().view(2, chw)
        for j, at in enumerate(spots):
            bad[:, at] = (math.nan, math.inf, -math.inf)[j % 3]
        mask = torch.zeros(2, chw, dtype=torch.bool)
        mask[:, spots] = True
        scales = torch.empty(2, device=dev)
        got = hip_ops.pred_to_eps_(bad.view(shape).to(dev), x.to(dev), t.to(dev), ah_d, pk, clip, out=torch.empty(shape, device=dev),
                                   x0_threshold=p, scale_out=scales).cpu().view(2, chw)
        assert not torch.isfinite(got[mask]).any() and torch.isfinite(got[~mask]).all(), (pk, inf_scale)
        static = hip_ops.pred_to_eps_(bad.view(shape).to(dev), x.to(dev), t.to(dev), ah_d, pk, clip,
                                      out=torch.empty(shape, device=dev)).cpu().view(2, chw)
        if inf_scale:
            assert torch.isinf(scales).all() and torch.equal(_bits(got[~mask]), _bits(static[~mask]))
            continue
        # the oracle on the implied x0 with the planted elements at +inf
        x0 = PO.to_x0(pk, pc.double(), x, ah, t).view(2, chw)
        x0[mask] = math.inf
        q, want_s = TO.threshold_x0(x0.view(shape), clip, p)
        a, s = PO.a_s(ah, t)
        want, bound = PO._over_s(x.double(), a * q, s)
        want, bound = want.view(2, chw), bound.view(2, chw)
        err = (got[~mask].double() - want[~mask]).abs().max().item() / bound[~mask].max().item()
        assert err <= KERNEL_BAR and torch.isfinite(scales).all()
        assert ((scales.cpu().double() - want_s).abs() <= SCALE_BAR * want_s).all()
        assert not torch.equal(got[~mask], static[~mask])


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------
def test_wrappers_reject_bad_arguments(dev, table):
    from diffusionremotesensing_amd import hip_ops
    ah, ah_d = table
    x = torch.zeros((2, 3, 8, 8), device=dev)
    p = torch.ones((2, 3, 8, 8), device=dev)
    t = torch.ones(2, dtype=torch.int64, device=dev)
    clip = (0.0, 1.0)
    with pytest.raises(RuntimeError, match="two buffers"):
        hip_ops.pred_to_eps_(x, x, t, ah_d, "v", clip, x0_threshold=0.5)  # x aliased to the result (in place)
    with pytest.raises(RuntimeError, match="two buffers"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, out=x, x0_threshold=0.5)
    with pytest.raises(ValueError, match="needs x0_clip"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", x0_threshold=0.5)
    with pytest.raises(ValueError, match="required"):
        hip_ops.x0_abs_quantile(p, x, t, ah_d, "v", None, 0.5)
    for bad in (0.0, -0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="x0_threshold"):
            hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, x0_threshold=bad)
        with pytest.raises(ValueError, match="x0_threshold"):
            hip_ops.x0_abs_quantile(p, x, t, ah_d, "v", clip, bad)
    with pytest.raises(ValueError, match="lo < hi"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", (1.0, 1.0), x0_threshold=0.5)
    with pytest.raises(ValueError, match="scale_out"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, scale_out=torch.empty(2, device=dev))
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(p, torch.zeros((2, 3, 8, 7), device=dev), t, ah_d, "v", clip, x0_threshold=0.5)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, x0_threshold=0.5, pred_uncond=torch.zeros((2, 3, 8, 7), device=dev))
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(p, x, torch.ones(3, dtype=torch.int64, device=dev), ah_d, "v", clip, x0_threshold=0.5)
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, x0_threshold=0.5, scale_out=torch.empty(3, device=dev))
    with pytest.raises(RuntimeError, match="scale_out"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, x0_threshold=0.5, scale_out=torch.empty(2, dtype=torch.float64, device=dev))
    with pytest.raises(RuntimeError, match="scale_out"):
        hip_ops.pred_to_eps_(p, x, t, ah_d, "v", clip, x0_threshold=0.5, scale_out=torch.empty(2))
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.pred_to_eps_(p, x, t, ah, "v", clip, x0_threshold=0.5)  # the table must live on the device
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.x0_abs_quantile(p.cpu(), x, t, ah_d, "v", clip, 0.5)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip_ops.pred_to_eps_(torch.zeros((2, 3, 8, 16), device=dev)[..., ::2], x, t, ah_d, "v", clip, x0_threshold=0.5)
    with pytest.raises(RuntimeError, match="int64"):
        hip_ops.pred_to_eps_(p, x, t.int(), ah_d, "v", clip, x0_threshold=0.5)
    with pytest.raises(RuntimeError, match="float32"):
        hip_ops.x0_abs_quantile(p.double(), x, t, ah_d, "v", clip, 0.5)
    assert torch.equal(p, torch.ones_like(p)) and torch.equal(x, torch.zeros_like(x))  # nothing was written
    assert hip_ops.x0_abs_quantile(p[:0], x[:0], t[:0], ah_d, "v", clip, 0.5).shape == (0,)


# ---------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------
# rel-L2 and PSNR (dB, on the [0, 1]-clamped images) of the thresholded chains (p = 0.995) against the float64 chains fed the
# oracle's thresholded eps, per family: (bound on rel-L2, bound on PSNR) = 10x the rel-L2 and 20 dB under the PSNR measured on
# MI355X for the family's worst case, the rule of BOUNDS in tests/test_gpu_prediction.py.  Measured (rel-L2 / PSNR):
#   superres v, clip (0, 1)              ancestral 2.2e-6 / 119.0 dB, DDIM 7 2.0e-6 / 120.4 dB, DPM-Solver++ 10 1.9e-6 / 120.5 dB
#   generation v, cfg 3, DDIM 7, (0, 1)  4.2e-6 / 113.4 dB      sample_known v DDIM 7, clip (0, 1)   1.5e-6 / 122.2 dB
#   tiler v DDIM 7, clip (0, 1)          per_step 2.5e-6 / 118.4 dB, final 2.2e-6 / 119.4 dB
#   Gaussian problem v, DDIM 10, (-1, 1) 3.7e-7 / 140.7 dB
# Every family lies inside its bound of tests/test_gpu_prediction.py: the threshold adds rounding of the conversion's order.
BOUNDS = {"superres": (2.2e-5, 99.0), "generation": (4.2e-5, 93.0), "known": (1.5e-5, 102.0), "tiler": (2.5e-5, 98.0),
          "gauss": (3.8e-6, 120.0)}
SAMPLERS = {"ancestral": ("ancestral",), "ddim7_eta0": ("ddim", 7, 0.0), "dpmpp10": ("dpmpp_2m", 10)}
P = 0.995


def _psnr_clamped(a, b):
    mse = ((a.double().clamp(0, 1) - b.double().clamp(0, 1)) ** 2).mean().item()
    return float("inf") if mse == 0 else -10 * math.log10(mse)


def _check_chain(family, what, got, want):
    e_max, e_l2 = rel_errors(got, want)
    psnr = _psnr_clamped(got, want)
    print(f"threshold chain {what}: max-rel {e_max:.3e} rel-L2 {e_l2:.3e} PSNR {psnr:.1f} dB (max |x| {want.abs().max():.3g})")
    assert torch.isfinite(got).all()
    assert e_l2 <= BOUNDS[family][0] and psnr >= BOUNDS[family][1], (what, e_l2, psnr)


def _sampling_args(sampler):
    from diffusionremotesensing_amd.sampling import sampling_plan
    if sampler[0] == "ancestral":
        return {}
    if sampler[0] == "ddim":
        return {"sampling_steps": sampler[1], "eta": sampler[2]}
    return {"sampling_steps": sampling_plan(sampler[1], solver="dpmpp_2m")}


@pytest.fixture(scope="module")
def model(dev, seeded_sd):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    return m


def _superres(model, dev, T=50, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", model, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                     image_size=64, Degradation_type="DownBlur", **kw)


class _StubEngine:
    def check_faults(self):
        pass


def _gauss_chain(dev, **attrs):
    """`sample_chain` on the optimal v predictor of per-pixel N(0, VAR0) data (no network), DDIM S = 10."""
    from diffusionremotesensing_amd import sampling
    T, S, shape = 50, 10, (2, 3, 16, 20)
    alpha, ah, beta = D.schedule("cosine", T)
    pred = PO.gauss_pred("v", ah)
    sched = types.SimpleNamespace(noise_steps=T, alpha=alpha.to(dev), alpha_hat=ah.to(dev), beta=beta.to(dev), device=dev,
                                  prediction="v", **attrs)

    def predict(engine, x, t, first):
        return pred(x.cpu(), int(t[0].item())).to(dev).contiguous()
    got = sampling.sample_chain(sched, _StubEngine(), shape, predict, table_rows=shape[0], noise_source=replay_noise_source(11),
                                sampling_steps=S, eta=0.0).cpu()
    return got, (T, S, shape, ah, pred)


def test_gaussian_problem_thresholded(dev):
    import ddim_oracle as O
    clip = (-1.0, 1.0)
    got, (T, S, shape, ah, pred) = _gauss_chain(dev, x0_clip=clip, x0_threshold=P)
    want = O.chain(TO.eps_fn_of("v", clip, P, ah, pred), shape, T, ah, S, 0.0, replay_noise_source(11))
    _check_chain("gauss", "gaussian v ddim10 clip=(-1, 1) p=0.995", got, want)
    static, _ = _gauss_chain(dev, x0_clip=clip)
    assert not torch.equal(got, static)  # the threshold bit somewhere along the chain


def test_a_threshold_that_never_exceeds_the_range_is_the_clip_chain(dev):
    """The data's standard deviation is 0.5 and every implied x0 is narrower: the median of |x0| stays under 1, every image of
    every step takes the static form, and the chain is the `x0_clip`-only chain bit for bit."""
    clip = (-1.0, 1.0)
    got, _ = _gauss_chain(dev, x0_clip=clip, x0_threshold=0.5)
    static, _ = _gauss_chain(dev, x0_clip=clip)
    assert torch.equal(_bits(got), _bits(static))


@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_superres_v_chain_vs_oracle(dev, model, seeded_sd, sampler):
    """n = 2, 64x64 (LR 32x32, x2), cosine T = 50, the seeded weights read as a v network, clip (0, 1), p = 0.995; the chains
    that draw nothing but x_T run twice, bit for bit."""
    from diffusionremotesensing_amd import synthetic
    clip = (0.0, 1.0)
    d = _superres(model, dev, prediction="v", x0_clip=clip, x0_threshold=P)
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    args = _sampling_args(SAMPLERS[sampler])
    x = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
    model.eval()
    if sampler in ("ddim7_eta0", "dpmpp10"):
        again = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
        model.eval()
        assert torch.equal(x, again)
    want = TO.chain("v", clip, P, PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2), (2, 3, 64, 64), 50,
                    D.schedule("cosine", 50), SAMPLERS[sampler], replay_noise_source(505))
    _check_chain("superres", f"superres v {sampler} clip=(0, 1) p={P}", x, want)
    d.x0_threshold = None  # a plain attribute: the next call is the clip-only chain
    plain = d.sample(2, model, lr1, input_channels=3, noise_source=replay_noise_source(505), **args).cpu()
    model.eval()
    assert not torch.equal(plain, x)


def test_generation_guided_v_chain_vs_oracle(dev, seeded_sd_gen):
    """cfg_scale = 3: the one conversion launch sequence forms the guided v, thresholds its x0 and hands the update one eps."""
    from diffusionremotesensing_amd.generate_new_imgs.train_diffusion_generation import Diffusion
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = Residual_Attention_UNet_generation(3, 3, 10, dev)
    m.load_state_dict(seeded_sd_gen)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(IMPL)
    clip = (0.0, 1.0)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, image_size=64, prediction="v",
                  x0_clip=clip, x0_threshold=P)
    cls = torch.tensor([2, 5])
    x = d.sample(2, m, target_class=cls, cfg_scale=3, input_channels=3, noise_source=replay_noise_source(202),
                 sampling_steps=7, eta=0.0).cpu()
    want = TO.chain("v", clip, P, PO.generation_pred_fn(U.OracleUNetGeneration(seeded_sd_gen), 2, cls, 3), (2, 3, 64, 64), 50,
                    D.schedule("cosine", 50), ("ddim", 7, 0.0), replay_noise_source(202))
    _check_chain("generation", f"generation v cfg=3 ddim7 clip=(0, 1) p={P}", x, want)


def test_sample_known_v_chain_vs_oracle(dev, model, seeded_sd):
    import inpaint_oracle as I
    from diffusionremotesensing_amd import synthetic
    clip = (0.0, 1.0)
    d = _superres(model, dev, prediction="v", x0_clip=clip, x0_threshold=P)
    lr1 = synthetic.tensor_uniform("ddim.sr.lr", (3, 32, 32))
    known = synthetic.tensor_uniform("prediction.known", (3, 64, 64))
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :24] = True
    x = d.sample_known(2, model, lr1, known, mask, input_channels=3, noise_source=replay_noise_source(606),
                       sampling_steps=7, eta=0.0).cpu()
    model.eval()
    sched = D.schedule("cosine", 50)
    eps_fn = TO.eps_fn_of("v", clip, P, sched[1], PO.superres_pred_fn(U.OracleUNet(seeded_sd), 2, lr1, 2))
    want = I.chain(eps_fn, (2, 3, 64, 64), 50, *sched, 7, 0.0, replay_noise_source(606), known, mask)
    assert torch.equal(x[:, :, :, :24], known[None, :, :, :24].expand(2, -1, -1, -1))
    _check_chain("known", f"sample_known v ddim7 clip=(0, 1) p={P}", x, want)


@pytest.mark.parametrize("mode", ["per_step", "final"])
def test_tiler_v_scene_vs_oracle(dev, model, seeded_sd, mode):
    """The 2 x 2-tile scene of tests/test_gpu_prediction.py with the threshold: the statistic is per tile, the image the
    network saw, in both modes."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T, S, clip = 50, 7, (0.0, 1.0)
    d = _superres(model, dev, T, prediction="v", x0_clip=clip, x0_threshold=P)
    img = synthetic.tensor_uniform("prediction.scene", (1, 3, 48, 48))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(48, 48, 32, 16, 2)
    lr_tiles = torch.stack([img[0, :, y0:y0 + 32, x0:x0 + 32] for (y0, x0) in lr_origins])
    sched = D.schedule("cosine", T)
    net = U.OracleUNet(seeded_sd)
    if mode == "per_step":
        tiler.tile_batch = 2
        got = tiler.sample_scene(noise_source=replay_noise_source(707), sampling_steps=S, eta=0.0).cpu()

        def eps_fn(x_tiles, t, rng):
            pred = net(x_tiles, torch.full((rng[1] - rng[0],), t, dtype=torch.long), lr_tiles[rng[0]:rng[1]], 2)
            return TO.to_eps("v", pred, x_tiles, sched[1], t, clip, P)[0]
        want = TC.chain(eps_fn, 3, 96, 96, infos, A.gaussian_weight(64, 64), T, sched, replay_noise_source(707), S, 0.0)
    else:
        from conftest import replay_tile_noise
        src = replay_tile_noise(808, 4, T, (1, 3, 64, 64))
        got = tiler.sample_tiles(noise_source=src, sampling_steps=S, eta=0.0).cpu()
        want = torch.cat([TO.chain("v", clip, P, PO.superres_pred_fn(net, 1, lr_tiles[k], 2), (1, 3, 64, 64), T, sched,
                                   ("ddim", S, 0.0), lambda i, shape, k=k: src(k, i, shape)) for k in range(4)])
    model.eval()
    _check_chain("tiler", f"tiler {mode} v ddim7 clip=(0, 1) p={P}", got, want)
