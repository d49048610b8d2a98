"""The blind-degradation ops on the GPU (csrc/bsr_degrade.hip through diffusionremotesensing_amd.bsr) against the float64 / integer
oracle of tests/bsr_oracle.py, the pipeline stage by stage, the feed and the trainer's --Degradation_type BSRGAN."""
import math
import re

import numpy as np
import pytest
import torch

import bsr_oracle as BO

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
# Bounds, derived and not measured; all in units of 2^-24 M with M = max |x| (1 where the input lies in [0, 1]).
#   blur      a chain of k^2 FMAs over non-negative weights that sum to 1: every partial sum is at most M, every FMA rounds once,
#             so the error is at most k^2 units (+ 2: the fp32 weights sum to 1 only to k^2 2^-25).
#   separable two chains of k FMAs; the column pass carries the row pass's error through weights that sum to 1: 2 k + 2.
#   USM       blur error e_b = 2 k + 2, soft-mask error e_s = 2 k + 2 (the mask is at most 1), sharp = clip(x + w (x - blur)) errs
#             by w e_b + 2, out = soft sharp + (1 - soft) x by |sharp - x| e_s + soft (w e_b + 2) + 3 with |sharp - x| <= w = 1/2:
#             2 k + 8.  The mask is a step: pixels within 255 (e_b + 2) units of the threshold are taken both ways (BO.usm).
#   resize    weights w = S-bounded rows (S = the oracle's largest sum |w| of the axis: 1 but for bicubic), T taps an axis; the two
#             FMA chains cost (T_x + T_y) S_x S_y, the fp32 weights E_x S_y + E_y S_x with E the axis's summed weight error: one
#             rounding per weight for bilinear and area (E = T), and for bicubic the Horner forms of the cubic (three steps on
#             magnitudes up to 12 with t <= 2: under 34 units a weight, 60 for the one formed as 1 - the others; E = 4 * 64).
def blur_units(k):
    return k * k + 2


def sep_units(k):
    return 2 * k + 2


def usm_units(k):
    return 2 * k + 8


def resize_units(h, w, h2, w2, mode):
    def axis(n_in, n_out):
        m = BO.axis_matrix(n_in, n_out, mode)
        taps = int((m != 0).sum(axis=1).max()) if not (mode == 2) else 4
        return taps, np.abs(m).sum(axis=1).max(), (4 * 64 if mode == 2 else taps)
    (ty, sy, ey), (tx, sx, ex) = axis(h, h2), axis(w, w2)
    return (tx + ty) * sx * sy + ex * sy + ey * sx + 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _rand(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def _kernels(n, k, seed):
    """n different non-negative k x k kernels, normalised: Gaussians of random widths times a random texture, not symmetric."""
    rng = np.random.default_rng(seed)
    t = np.arange(k) - k // 2
    out = np.empty((n, k, k), dtype=np.float32)
    for i in range(n):
        sy, sx = rng.uniform(0.8, k / 3, 2)
        kk = np.exp(-t[:, None] ** 2 / (2 * sy * sy) - t[None, :] ** 2 / (2 * sx * sx)) * rng.uniform(0.5, 1.5, (k, k))
        out[i] = kk / kk.sum()
    return torch.from_numpy(out)


def _units(got, want, M):
    return (np.abs(got.double().cpu().numpy() - want).max() / (EPS * M)).item()


BLUR_CASES = [((1, 1, 1, 1), 7),      # every tap reflects onto the one pixel
              ((1, 1, 5, 7), 25),     # the image is smaller than the 12-pixel halo: the reflection repeats
              ((2, 3, 33, 47), 7), ((2, 3, 33, 47), 15),  # odd sizes, a different kernel per image
              ((1, 16, 40, 72), 25),  # 16 bands, two tiles across and down
              ((1, 3, 130, 200), 11)]  # several tiles both ways


@pytest.mark.parametrize("shape,k", BLUR_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"k{v}")
def test_blur_vs_float64_oracle(dev, shape, k):
    """|got - want| <= (k^2 + 2) 2^-24 max |x| against the true convolution on the reflect-101 border.
    Measured on MI355X, units of 2^-24 max |x|, in the order of BLUR_CASES: 0.06 / 4.08 / 4.32 / 7.46 / 15.87 / 6.31."""
    from diffusionremotesensing_amd import bsr
    x, ker = _rand(shape, 3 + sum(shape), -0.2, 1.2), _kernels(shape[0], k, 5 + k)
    got = bsr.blur(x.to(dev), ker.to(dev))
    assert got.shape == x.shape and got.dtype == torch.float32
    u = _units(got, BO.blur(x, ker), x.abs().max().item())
    print(f"blur {shape} k={k}: {u:.2f} of {blur_units(k)} units")
    assert u <= blur_units(k)
    flipped = _units(got, BO.blur(x, ker.flip(1, 2)), x.abs().max().item())
    assert min(shape[2:]) < 5 or flipped > 1e3  # a correlation instead of a convolution is far outside


def test_blur_with_a_kernel_size_per_image(dev):
    """(2, 3, 33, 47): image 0 under a 7 x 7, image 1 under a 15 x 15 kernel, both centred in one 15 x 15 table; what lies outside
    image 0's 7 x 7 part is not read (it is filled with ones here)."""
    from diffusionremotesensing_amd import bsr
    shape = (2, 3, 33, 47)
    x = _rand(shape, 41, -0.2, 1.2)
    table = torch.ones((2, 15, 15))
    table[0, 4:11, 4:11] = _kernels(1, 7, 42)[0]
    table[1] = _kernels(1, 15, 43)[0]
    ksizes = torch.tensor([7, 15], dtype=torch.int32)
    got = bsr.blur(x.to(dev), table.to(dev), ksizes.to(dev))
    u = _units(got, BO.blur(x, table, ksizes.tolist()), x.abs().max().item())
    print(f"blur per-image sizes: {u:.2f} units")
    assert u <= blur_units(15)
    assert _units(got[:1], BO.blur(x[:1], table[:1, 4:11, 4:11]), x.abs().max().item()) <= blur_units(7)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 5, 7), (2, 3, 33, 47), (1, 3, 130, 200)], ids=lambda s: "x".join(map(str, s)))
def test_separable_blur_and_usm_vs_float64_oracle(dev, shape):
    """The 51-tap sigma-8 Gaussian (the halo of 25 exceeds the two small images: repeated reflection) and a 9-tap asymmetric kernel,
    then the USM: the result lies between the oracle's two resolutions of the threshold pixels, to (2 k + 8) units.
    Measured on MI355X, 51 taps / 9 taps / USM excess, (1,1,1,1): 0.73 / 0.33 / 0.00, (1,1,5,7): 3.05 / 0.86 / 1.88, (2,3,33,47):
    3.95 / 1.99 / 2.21, (1,3,130,200): 4.73 / 2.36 / 2.58 (7188 of its 78000 pixels lie within 25 pixels of a threshold pixel)."""
    from diffusionremotesensing_amd import bsr
    x = _rand(shape, 7 + sum(shape))
    xd = x.to(dev)
    lop = np.random.default_rng(2).random(9).astype(np.float32)
    lop /= lop.sum()
    for taps in (bsr.usm_taps(), lop):
        k = len(taps)
        u = _units(bsr.blur_sep(xd, taps), BO.blur_sep(x, taps), 1.0)
        print(f"blur_sep {shape} k={k}: {u:.2f} of {sep_units(k)} units")
        assert u <= sep_units(k)
    taps, k = bsr.usm_taps(), 51
    got = bsr.sharpen(xd).double().cpu().numpy()
    lo, hi = BO.usm(x, taps, 0.5, 10.0, ambiguous=255 * (sep_units(k) + 2) * EPS)
    print(f"usm {shape}: {int((hi > lo).sum())} pixels feel a threshold pixel; worst excess "
          f"{max((lo - got).max(), (got - hi).max()) / EPS:.2f} of {usm_units(k)} units")
    assert (got >= lo - usm_units(k) * EPS).all() and (got <= hi + usm_units(k) * EPS).all()
    if min(shape[2:]) >= 33:
        assert np.abs(got - x.double().numpy()).max() > 0.01  # it does sharpen
    assert got.min() >= 0 and got.max() <= 1


RESIZE_CASES = [((2, 3, 33, 47), (16, 23)), ((2, 3, 33, 47), (50, 71)), ((2, 3, 33, 47), (1, 1)), ((1, 2, 8, 8), (8, 8)),
                ((1, 1, 130, 200), (97, 301))]  # (the last: shrinking down, enlarging across)


@pytest.mark.parametrize("mode", [1, 2, 3], ids=["bilinear", "bicubic", "area"])
@pytest.mark.parametrize("shape,out", RESIZE_CASES, ids=lambda v: "x".join(map(str, v)))
def test_resize_vs_float64_oracle(dev, shape, out, mode):
    """Input in [-0.2, 1.2] so that the fused clip acts; the same size is the identity (after the clip) bit for bit; the quantised
    copy is rint(out * 255) / 255 of the kernel's own result.
    Measured on MI355X, worst over the shapes: bilinear 2.06 of 10 units, bicubic 15.06 of 721, area 1.98 of 12."""
    from diffusionremotesensing_amd import bsr
    x = _rand(shape, 9 + sum(shape) + mode, -0.2, 1.2)
    got, got_q = bsr.resize(x.to(dev), out[0], out[1], mode, quantise=True)
    assert got.shape == shape[:2] + out and got.min().item() >= 0 and got.max().item() <= 1
    bound = resize_units(shape[2], shape[3], out[0], out[1], mode)
    u = _units(got, BO.resize(x, out[0], out[1], mode), x.abs().max().item())
    print(f"resize {shape} -> {out} mode {mode}: {u:.2f} of {bound:.0f} units")
    assert u <= bound
    assert np.array_equal(got_q.cpu().numpy(), BO.quantise(got))
    assert torch.equal(bsr.resize(x.to(dev), out[0], out[1], mode), got)
    if shape[2:] == out:
        assert torch.equal(got.cpu(), x.clamp(0, 1))
    elif out != (1, 1):
        other = BO.resize(x, out[0], out[1], 1 if mode == 2 else 2)
        assert _units(got, other, x.abs().max().item()) > 1e3  # the modes differ by far more than the bound


def _noise_case(n, c, seed):
    """Image i of the batch: kind / branch cycle through every combination; sigma level / 255; a full covariance factor."""
    from diffusionremotesensing_amd import bsr
    rng = np.random.default_rng(seed)
    combos = [(0, 0)] + [(k, b) for k in (1, 2) for b in (0, 1, 2)]
    mode = np.array([combos[i % len(combos)] for i in range(n)], dtype=np.int32)
    par = np.zeros((n, 10), dtype=np.float32)
    par[:, 0] = rng.integers(2, 26, n) / 255.0
    par[:, 1:] = np.stack([bsr.covariance_factor(rng) for _ in range(n)]).reshape(n, 9)
    return torch.from_numpy(mode), torch.from_numpy(par)


def _noise_units(x, z, mode, par, got, want, aux=None):
    """The worst error of drs_bsr_noise per image, in the units its tests derive: 2^-24 (|x| + (1 + |x|) |nv|) with |nv| taken as
    sigma |z| or sum_j |A_ij| |z_j| for the Gaussian kinds, 2^-24 (1 + |z - rate| / vals) for the Poisson kinds."""
    xx, zz, got = x.double().numpy(), z.double().numpy(), got.double().numpy()
    c, out = xx.shape[1], {}
    for i in range(xx.shape[0]):
        kind, branch = mode[i].tolist()
        A, sigma = par[i, 1:].double().numpy().reshape(3, 3), par[i, 0].item()
        if kind == 0 or (kind == 4 and aux is None):
            assert np.array_equal(got[i], xx[i])
            continue
        if kind in (3, 4):
            d = np.abs(zz[i, :1] - (aux[i].double().numpy()[None] if kind == 4 else 0.0)) / sigma
            scale = EPS * (1 + d) * np.ones_like(xx[i])
        else:
            if branch == 0 or (branch == 2 and c != 3):
                nabs = np.abs(sigma * zz[i])
            elif branch == 1:
                nabs = np.broadcast_to(np.abs(sigma * zz[i, 0]), xx[i].shape)
            else:
                nabs = np.einsum("ij,jhw->ihw", np.abs(A), np.abs(zz[i]))
            scale = EPS * (np.abs(xx[i]) + (1 + np.abs(xx[i])) * nabs)
        out[i] = (np.abs(got[i] - want[i]) / scale).max()
    return out


@pytest.mark.parametrize("c", [3, 5])
def test_noise_every_branch_with_given_draws(dev, c):
    """8 images (off, then additive and speckle x per band / one plane / correlated) of 19 x 23 with z given.  Per element, with nv
    the noise value: sigma z and the sum are two roundings, the correlated form three FMAs, the speckle FMA one more on |x nv + x|
    - at most 4 units of 2^-24 (|x| + (1 + |x|) sum_j |A_ij z_j|).  The image whose op is off keeps its bits; c = 5 takes the
    correlated branch as per band.  Measured on MI355X: at most 1.41 of the 4 units."""
    from diffusionremotesensing_amd import bsr
    n = 8
    x, z = _rand((n, c, 19, 23), 60 + c, -0.1, 1.1), torch.randn((n, c, 19, 23), generator=torch.Generator().manual_seed(61))
    mode, par = _noise_case(n, c, 62)
    xd = x.to(dev)
    out = bsr.noise_(xd, z.to(dev), mode.to(dev), par.to(dev))
    assert out is xd
    got = xd.cpu()
    want = BO.noise(x, z, mode, par)
    assert torch.equal(got[0], x[0]) and torch.equal(got[7], x[7])  # (mode 7 % 7 = 0: off again)
    for i, u in _noise_units(x, z, mode, par, got, want).items():
        print(f"noise c={c} image {i} kind/branch {mode[i].tolist()}: {u:.2f} of 4 units")
        assert u <= 4
        assert np.abs(want[i] - x[i].clamp(0, 1).double().numpy()).max() > 1e-3 and got[i].min() >= 0 and got[i].max() <= 1


def _check_rate(rate, x, mode, par):
    """`bsr.poisson_rate` (a torch composition, no kernel) against the oracle's float32 restatement: torch's division by a scalar on
    the device may multiply by the reciprocal, so the rate is held to 4 fp32 roundings, and the integer LEVEL it encodes - what
    the gray formula and the quantisation decide - to equality."""
    want = BO.poisson_rate(x, mode, par).astype(np.float64)
    got = rate.double().cpu().numpy()
    assert (np.abs(got - want) <= 4 * EPS * want).all()
    vals = par[:, 0].double().numpy().reshape(-1, 1, 1, 1)
    assert np.array_equal(np.rint(got / vals * 255), np.rint(want / vals * 255))


def test_poisson_combination(dev):
    """Kinds 3 and 4 with given draws: x = clip(z / vals) per band; x = clip(q(x) + (z0 - rate) / vals) for the gray kind, whose rate
    plane comes from `poisson_rate` (`_check_rate`).  Division, difference and sum
    round once each on magnitudes up to 1 + |d|: 4 units of 2^-24 (1 + |z - rate| / vals).  Measured on MI355X: 0.51."""
    from diffusionremotesensing_amd import bsr
    n, c = 4, 3
    x = _rand((n, c, 17, 21), 70)
    mode = torch.tensor([[3, 0], [4, 0], [0, 0], [4, 0]], dtype=torch.int32)
    par = torch.zeros((n, 10))
    par[:, 0] = torch.tensor([150.0, 3000.0, 500.0, 101.5])
    rate = bsr.poisson_rate(x.to(dev), mode.to(dev), par.to(dev))
    _check_rate(rate, x, mode, par)
    z = torch.poisson(rate.cpu(), generator=torch.Generator().manual_seed(71))
    aux = rate[:, 0].contiguous()
    xd = x.to(dev)
    bsr.noise_(xd, z.to(dev), mode.to(dev), par.to(dev), aux)
    got, want = xd.cpu(), BO.noise(x, z, mode, par, aux.cpu())
    assert torch.equal(got[2], x[2])
    units = _noise_units(x, z, mode, par, got, want, aux.cpu())
    print(f"poisson: {units} of 4 units")
    assert set(units) == {0, 1, 3} and max(units.values()) <= 4
    assert np.abs(want[0] - x[0].numpy()).max() > 0.01 and np.abs(want[1] - x[1].numpy()).max() > 1e-3
    same = x.to(dev)
    bsr.noise_(same, z.to(dev), mode.to(dev), par.to(dev))  # without the rate plane the gray kind writes nothing
    assert torch.equal(same[1].cpu(), x[1]) and torch.equal(same[0].cpu(), got[0])


JPEG_SHAPES = [(1, 3, 8, 8), (2, 3, 16, 16), (1, 3, 24, 40), (1, 3, 37, 53), (3, 3, 48, 64)]


def _textured(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    f = torch.rand((n, c, 3, 1, 1), generator=g)
    img = 0.5 + 0.25 * torch.sin(0.7 * f[:, :, 0] * y + 0.7 * f[:, :, 1] * x + 6 * f[:, :, 2]) + 0.15 * ((x // 5 + y // 7) % 2) \
        + 0.06 * torch.randn(shape, generator=g)
    return img  # (leaves [0, 1] in places: the codec's own clip acts)


@pytest.mark.parametrize("shape", JPEG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_jpeg_equals_the_integer_oracle_to_the_bit(dev, shape):
    """Per-image qualities across 30 .. 95 (and the ends 1 and 100 of the rule in a second pass); partial MCUs at 8 x 8, 24 x 40
    and 37 x 53."""
    from diffusionremotesensing_amd import bsr
    x = _textured(shape, 80 + shape[2])
    for qs in ([30, 62, 95], [100, 1, 50]):
        q = torch.tensor(qs[:shape[0]], dtype=torch.int32)
        got = bsr.jpeg(x.to(dev), q.to(dev)).cpu().numpy()
        want = BO.jpeg(x, q.tolist())
        diff = np.abs(got - want) * 255
        print(f"jpeg {shape} q={q.tolist()}: {int((diff > 0).sum())} of {diff.size} values differ, worst {diff.max():.1f} levels")
        assert np.array_equal(got, want)
        assert qs[0] != 30 or np.abs(got - x.clamp(0, 1).numpy()).max() > 0.02  # (it is not the identity)


def _on_grid(t):
    """Every value is float32(k) / float32(255), k = 0 .. 255 (formed with numpy on the host: a true division)."""
    return np.array_equal(BO.quantise(t.cpu()), t.cpu().numpy())


def _forced_recipe(kind, seed):
    """A drawn recipe for 2 x 3 x 64 x 64, m = 2, with the rare per-image ops switched on for image 0 (and off for image 1), the two
    Poisson slots one per band and one gray - `degrade` applies whatever recipe it is given."""
    from diffusionremotesensing_amd import bsr
    r = bsr.draw_recipe(np.random.default_rng(seed), 2, 3, 64, 64, 2, kind)
    grays = iter([False, True])
    for op in r["ops"]:
        if op["op"] in ("speckle", "poisson"):
            op["on"] = np.array([True, False])
        if op["op"] == "poisson":
            op["gray"] = np.array([next(grays), False])
    return r


@pytest.mark.parametrize("kind,seed", [("plus", 1), ("plus", 2), ("soft", 3)])
def test_pipeline_stage_by_stage(dev, kind, seed):
    """`degrade(..., return_intermediates=True)`: every stage against the oracle applied to the GPU's OWN previous intermediate
    (a one-level flip in front of a JPEG does not become a block-sized difference downstream), with the bounds of the op tests."""
    from diffusionremotesensing_amd import bsr
    recipe = _forced_recipe(kind, seed)
    hr = _textured((2, 3, 64, 64), 90 + seed).clamp(0, 1).to(dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    lr, hr_out, stages = bsr.degrade(hr, recipe, return_intermediates=True, generator=gen)
    assert lr.shape == (2, 3, 32, 32) and lr.min().item() >= 0 and lr.max().item() <= 1
    assert _on_grid(lr)
    seen = []
    for st in stages:
        inp, out, op = st["inp"].cpu(), st["out"].cpu(), st["params"]
        seen.append(st["op"])
        if st["op"] == "sharpen":
            assert torch.equal(st["out"], hr_out) and torch.equal(st["inp"], hr)
            lo, hi = BO.usm(inp, bsr.usm_taps(), 0.5, 10.0, ambiguous=255 * (sep_units(51) + 2) * EPS)
            got = out.double().numpy()
            assert (got >= lo - usm_units(51) * EPS).all() and (got <= hi + usm_units(51) * EPS).all()
        elif st["op"] == "blur":
            u = _units(out, BO.blur(inp, op["kernels"], op["ksize"].tolist()), 1.0)
            assert u <= blur_units(int(op["ksize"].max())), (st["slot"], u)
        elif st["op"] == "resize":
            assert out.shape[2:] == (op["out_h"], op["out_w"])
            u = _units(out, BO.resize(inp, op["out_h"], op["out_w"], op["mode"]), 1.0)
            assert u <= resize_units(inp.shape[2], inp.shape[3], op["out_h"], op["out_w"], op["mode"]), (st["slot"], u)
        elif st["op"] == "quantise":
            assert np.array_equal(out.numpy(), BO.quantise(inp))
        elif st["op"] == "jpeg":
            assert np.array_equal(out.numpy(), BO.jpeg(inp, op["quality"].tolist())), st["slot"]
        elif st["op"] in ("noise", "speckle", "poisson"):
            aux = st["aux"].cpu() if st["aux"] is not None else None
            want = BO.noise(inp, st["z"].cpu(), st["mode"].cpu(), st["par"].cpu(), aux)
            units = _noise_units(inp, st["z"].cpu(), st["mode"].cpu(), st["par"].cpu(), out, want, aux)
            assert units and max(units.values()) <= 4, (st["op"], units)
            assert torch.equal(out[1], inp[1]) or st["op"] == "noise"  # the image whose op is off keeps its bits
            if st["op"] == "poisson":
                _check_rate(st["rate"], inp, st["mode"].cpu(), st["par"].cpu())
                assert torch.equal(st["rate"][:, 0].cpu(), aux)
        else:
            raise AssertionError(st["op"])
        print(f"pipeline {kind}/{seed}: slot {st['slot']} {st['op']} ok")
    assert torch.equal(stages[-1]["out"], lr)
    if kind == "plus":
        assert seen[0] == "sharpen" and seen[-2:] == ["resize", "jpeg"] and {"blur", "noise", "speckle", "poisson"} <= set(seen)
        assert not torch.equal(hr_out, hr)
    else:
        assert seen[-2:] == ["resize", "quantise"] and "jpeg" not in seen and "sharpen" not in seen and torch.equal(hr_out, hr)
    again = bsr.degrade(hr, recipe, generator=torch.Generator(device=dev).manual_seed(seed))
    assert torch.equal(again[0], lr) and torch.equal(again[1], hr_out)


def test_thirteen_bands_run_without_jpeg(dev):
    from diffusionremotesensing_amd import bsr
    hr = _rand((2, 13, 32, 32), 5).to(dev)
    recipe = bsr.draw_recipe(np.random.default_rng(4), 2, 13, 32, 32, 4, "plus")
    lr, hr_out = bsr.degrade(hr, recipe, generator=torch.Generator(device=dev).manual_seed(1))
    assert lr.shape == (2, 13, 8, 8) and _on_grid(lr) and hr_out.shape == hr.shape
    with pytest.raises(RuntimeError, match="ROCm"):
        bsr.degrade(hr.cpu(), recipe)
    with pytest.raises(RuntimeError, match="3 bands"):
        bsr.jpeg(hr, torch.full((2,), 50, dtype=torch.int32, device=dev))


def _cache(dev, n=8, size=64):
    return (_textured((n, 3, size, size), 123).clamp(0, 1) * 255).round().to(torch.uint8).to(dev)


def test_feed_is_seeded_fixed_feeds_repeat_training_feeds_do_not(dev):
    from diffusionremotesensing_amd.bsr import DeviceBSRFeed
    u8 = _cache(dev)

    def run(feed):
        return [(x.clone(), y.clone()) for x, y in feed]
    a, b = DeviceBSRFeed(u8, 2, 4, True, "plus", 7), DeviceBSRFeed(u8, 2, 4, True, "plus", 7)
    ea, eb = run(a), run(b)
    assert len(a) == 2 and len(ea) == 2
    for (xa, ya), (xb, yb) in zip(ea, eb):
        assert xa.shape == (4, 3, 32, 32) and ya.shape == (4, 3, 64, 64) and xa.dtype == ya.dtype == torch.float32
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert 0 <= xa.min().item() and xa.max().item() <= 1 and 0 <= ya.min().item() and ya.max().item() <= 1
    second = run(a)
    assert not all(torch.equal(p[0], q[0]) for p, q in zip(ea, second))  # a training feed: a fresh degradation every epoch
    other = run(DeviceBSRFeed(u8, 2, 4, True, "plus", 8))
    assert not all(torch.equal(p[0], q[0]) for p, q in zip(ea, other))
    fixed = DeviceBSRFeed(u8, 2, 4, False, "soft", 7, fixed=True)
    f1, f2 = run(fixed), run(fixed)
    for (x1, y1), (x2, y2) in zip(f1, f2):
        assert torch.equal(x1, x2) and torch.equal(y1, y2)
    assert np.array_equal(f1[0][1].cpu().numpy(), u8[:4].cpu().numpy().astype(np.float32) / np.float32(255))  # soft: the cached images, in order
    x0, y0 = a.item(3)
    x1, y1 = a.item(3)
    assert x0.shape == (3, 32, 32) and y0.shape == (3, 64, 64) and torch.equal(x0, x1) and torch.equal(y0, y1)


def test_trainer_runs_two_steps_under_bsrgan(dev, tmp_path, monkeypatch, capsys):
    """`--Degradation_type BSRGAN --dataset_path synthetic_u8:8`, image_size 64, batch 4: one epoch of two steps, validation, the
    final sampling on the first five training images.  (NotImplementedError before the feed existed.)"""
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    T.main(["--epochs", "1", "--batch_size", "4", "--image_size", "64", "--model_name", "bsr_test", "--noise_steps", "6",
            "--loss", "MSE", "--magnification_factor", "2", "--dataset_path", "synthetic_u8:8", "--Degradation_type", "BSRGAN",
            "--check_preds_epoch", "1", "--bsr_seed", "3"])
    text = capsys.readouterr().out
    loss = float(re.search(r"Epoch 0: Running Train \(MSE\) (\S+)", text).group(1))
    val = float(re.search(r"Epoch 0: Running Val loss \(MSE\)\s*(\S+)", text).group(1))
    print(f"trainer under BSRGAN: train loss {loss}, validation loss {val}")
    assert math.isfinite(loss) and math.isfinite(val) and loss > 0
    res = torch.load(tmp_path / "models_run" / "bsr_test" / "results" / "superres_results.pt")
    assert res.shape == (5, 3, 64, 64) and torch.isfinite(res).all()
