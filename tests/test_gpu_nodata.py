"""No-data pixels on the GPU (csrc/nodata.hip and the MASKED kernels of csrc/loss.hip and csrc/metrics.hip, through hip_ops /
losses / metrics / the SAR -> NDVI trainer) against the float64 oracle of tests/nodata_oracle.py and against the unmasked
siblings.  The guard-band runs of the four entry points are in tests/test_gpu_entry_guards_nodata.py, whose name puts them in
front of tests/test_gpu_guard.py's census of the ABI."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import nodata_oracle as NO
import test_gpu_loss as GL
import test_gpu_metrics as GM
from guard import bits_equal

pytestmark = pytest.mark.gpu

A = (3, 3, 37, 41)        # C hw = 4551: crosses a 4096 chunk, hw % 4 != 0, band boundaries off the 16-byte grid
V1, V2 = (2, 1, 16, 16), (2, 16, 12, 28)  # the vector path
S = (5, 2, 11, 11)        # SSIM at its one window
T = GL.T
VALUE = 0.25              # the no-data value of the value-rule cases (no valid pixel holds it in every band)
JUNK = (math.nan, math.inf, -math.inf, 1e30)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _nodata(shape):
    """(B, H, W) bool, True = no-data: seeded blocks plus isolated pixels, and per batch size the three special images -
    B = 2: [fully valid, blocks]; B = 3: [blocks, no valid pixel, only the last pixel]; B = 5: [fully valid, none, last, blocks,
    one isolated pixel]."""
    B, _, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))

    def blocks():
        m = torch.zeros(H, W, dtype=torch.bool)
        for _ in range(3):
            y, x = int(torch.randint(0, H - 2, (1,), generator=g)), int(torch.randint(0, W - 2, (1,), generator=g))
            m[y:y + max(H // 4, 2), x:x + max(W // 3, 2)] = True
        m |= torch.rand(H, W, generator=g) < 0.03
        m[0, 0] = True  # (the first pixel)
        return m

    def last():
        m = torch.zeros(H, W, dtype=torch.bool)
        m[-1, -1] = True
        return m

    def isolated():
        m = torch.zeros(H, W, dtype=torch.bool)
        m[H // 2, W // 2] = True
        return m
    full, none = torch.zeros(H, W, dtype=torch.bool), torch.ones(H, W, dtype=torch.bool)
    return torch.stack({2: [full, blocks()], 3: [blocks(), none, last()], 5: [full, none, last(), blocks(), isolated()]}[B])


@functools.lru_cache(maxsize=None)
def _marked(shape, rule, seed=0):
    """A seeded fp32 image batch in (0, 1) whose no-data pixels (`_nodata`) carry the marker of `rule`: "nan" - a NaN in a
    seeded non-empty choice of bands; "value" - VALUE in all bands."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + len(rule))
    x = torch.rand(shape, generator=g) * 0.98 + 0.01
    nd = _nodata(shape)
    if rule == "value":
        return torch.where(nd[:, None], torch.full_like(x, VALUE), x)
    bands = torch.rand(shape, generator=g) < 0.5
    bands[:, 0] |= ~bands.any(dim=1)  # at least one band
    return torch.where(nd[:, None] & bands, torch.full_like(x, math.nan), x)


def _rule_value(rule):
    return True if rule == "nan" else VALUE


def _junk_like(x, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(JUNK)[torch.randint(0, len(JUNK), x.shape, generator=g)]


def _schedule(dev=None):
    steps = torch.arange(T) / T
    f = torch.cos(((steps + 0.008) / 1.008) * torch.pi / 2) ** 2
    return (f / f[0]).to(torch.float32)


# ---- identity with the unmasked siblings ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [A, V1, V2], ids=str)
def test_noise_identity(dev, shape):
    """Without a no-data pixel x_t is `noise_images`', the target eps, `noise_v_target`'s v or x0, the mask all ones - under the
    NaN rule and under a value no pixel holds."""
    from diffusionremotesensing_amd import hip_ops
    g = torch.Generator().manual_seed(3)
    x0, eps = torch.rand(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    t, ah = torch.randint(1, T, (shape[0],), generator=g).to(dev), _schedule().to(dev)
    want_xt = hip_ops.noise_images(x0, eps, t, ah)
    vx, v = hip_ops.noise_v_target(x0, eps, t, ah)
    assert torch.equal(vx, want_xt)
    for value in (None, -7.0):
        for kind, want in (("eps", eps), ("v", v), ("x0", x0)):
            x_t, target, valid = hip_ops.noise_target_nodata(x0, eps, t, ah, kind, value)
            assert torch.equal(x_t, want_xt) and torch.equal(target, want), (kind, value)
            assert valid.shape == (shape[0], 1) + shape[2:] and valid.dtype == torch.uint8 and bool((valid == 1).all())


@pytest.mark.parametrize("kind", GL.O.KINDS)
@pytest.mark.parametrize("shape", [A, V1, V2], ids=str)
def test_loss_identity(dev, shape, kind):
    """With every pixel valid every output - loss, its double, gradient, per-image losses, bins and ring - has the bits of
    `drs_diffusion_loss` on the same inputs, weighted and binned, with and without a gradient."""
    from diffusionremotesensing_amd.losses import DiffusionLoss, LossBins
    pred, target, t, table, sample_w = (x.to(dev) for x in GL._inputs(shape))
    valid = torch.ones((shape[0], 1) + shape[2:], dtype=torch.uint8, device=dev)
    for weighted in (False, True):
        outs = []
        for masked in (False, True):
            bins = LossBins(T, 4, dev)
            fn = DiffusionLoss(kind, table if weighted else None, bins, delta=GL.DELTA)
            kw = {"valid": valid} if masked else {}
            loss, grad = fn.loss_and_grad(pred, target, t, sample_w if weighted else None, **kw)
            with torch.no_grad():
                again = fn(pred, target, t, sample_w if weighted else None, **kw)
            outs.append((loss.clone(), grad, fn.per_image, fn.loss_f64.clone(), bins.buf, again))
            if masked:
                assert fn.valid_counts.tolist() == [shape[2] * shape[3]] * shape[0]
            else:
                assert fn.valid_counts is None
        for a, b in zip(*outs):
            assert bits_equal(a, b), (kind, weighted)


@pytest.mark.parametrize("shape", [A, V1, V2, S], ids=str)
def test_metrics_identity(dev, shape):
    from diffusionremotesensing_amd import hip_ops
    for content in ("noise", "bright_flat"):
        sr, hr = (x.to(dev) for x in GM._pair(shape, content))
        for clamp in (True, False):
            for nodata in (True, -7.0):
                sums = hip_ops.metrics_pointwise_nodata(sr, hr, nodata, clamp)
                C = shape[1]
                assert bits_equal(sums[:, :2 * C + 2].contiguous(), hip_ops.metrics_pointwise(sr, hr, clamp))
                assert sums[:, -1].tolist() == [shape[2] * shape[3]] * shape[0]
                s = hip_ops.ssim_nodata(sr, hr, nodata, clamp)
                assert bits_equal(s[:, 0].contiguous(), hip_ops.ssim_mean(sr, hr, clamp))
                assert s[:, 1].tolist() == [(shape[2] - 10) * (shape[3] - 10)] * shape[0]


# ---- against the float64 oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["nan", "value"])
@pytest.mark.parametrize("shape", [A, V1, V2], ids=str)
def test_noise_vs_oracle(dev, shape, rule):
    """The mask is the oracle's; at no-data pixels the target is +0.0 and x_t the noised fill; x_t and the v target lie within
    the three fp32 roundings (two products, one sum) of the oracle; a t outside the table gives NaN and no valid
    pixel; two calls give the same bits."""
    from diffusionremotesensing_amd import hip_ops
    x0 = _marked(shape, rule)
    g = torch.Generator().manual_seed(5)
    eps, ah = torch.randn(shape, generator=g), _schedule()
    t = torch.randint(1, T, (shape[0],), generator=g)
    bad = 0 if shape[0] == 2 else 1  # outside the table: the fully valid image of a pair, else the one without a valid pixel
    t[bad] = T
    live = [i for i in range(shape[0]) if i != bad]
    value = None if rule == "nan" else VALUE
    for kind in ("eps", "v", "x0"):
        got = hip_ops.noise_target_nodata(x0.to(dev), eps.to(dev), t.to(dev), ah.to(dev), kind, value, fill=0.3)
        again = hip_ops.noise_target_nodata(x0.to(dev), eps.to(dev), t.to(dev), ah.to(dev), kind, value, fill=0.3)
        assert all(bits_equal(a, b) for a, b in zip(got, again))
        x_t, target, valid = (v.cpu() for v in got)
        want_xt, want_target, want_valid = NO.noise_target(x0, eps, t, ah, kind, value, fill=0.3)
        assert torch.equal(valid[:, 0].bool(), want_valid) and int(valid.max()) <= 1
        assert torch.isnan(x_t[bad]).all() and torch.isnan(target[bad]).all() and not valid[bad].any()
        nd = ~want_valid[live][:, None].expand(len(live), *shape[1:])
        assert nd.any() and not nd.all()
        assert bool((target[live][nd] == 0).all()) and not torch.signbit(target[live][nd]).any()
        a = torch.sqrt(ah[t[live]]).double().view(-1, 1, 1, 1)
        b = torch.sqrt(1 - ah[t[live]]).double().view(-1, 1, 1, 1)
        xin = torch.where(nd, torch.full_like(x0[live], 0.3), x0[live]).double()
        # three roundings of 2^-24 each, relative to |a x| + |b eps| at most; 2^-22: one to spare
        bound = 2.0 ** -22 * ((a * xin).abs() + (b * eps[live].double()).abs())
        assert bool(((x_t[live].double() - want_xt[live]).abs() <= bound).all()), kind
        tb = 2.0 ** -22 * ((a * eps[live].double()).abs() + (b * xin).abs())
        assert bool(((target[live].double() - want_target[live]).abs() <= tb).all()), kind


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
@pytest.mark.parametrize("kind", GL.O.KINDS)
@pytest.mark.parametrize("shape", [A, V1, V2], ids=str)
def test_loss_vs_oracle(dev, shape, kind, weighted):
    """Per-image losses and the loss within test_gpu_loss.SUM_RTOL, the gradient under that file's element-wise bar and exactly
    +0.0 at no-data elements, the counts exact; junk under the mask changes no output bit; two calls give the same bits."""
    from diffusionremotesensing_amd.losses import DiffusionLoss
    pred, target, t, table, sample_w = GL._inputs(shape)
    nd = _nodata(shape)
    valid = (~nd).to(torch.uint8)[:, None].contiguous()
    w = GL.O.image_weights(shape[0], t, table, sample_w) if weighted else None
    per_image, loss, grad, counts, Bv = NO.masked_loss(pred, target, ~nd, kind, GL.DELTA, w)
    assert Bv == int((counts > 0).sum()) and (Bv < shape[0]) == (shape[0] == 3)  # (B = 3 holds the image without a valid pixel)
    fn = DiffusionLoss(kind, table.to(dev) if weighted else None, delta=GL.DELTA)
    args = (t.to(dev), sample_w.to(dev)) if weighted else ()

    def run(p, q):
        got_loss, got_grad = fn.loss_and_grad(p.to(dev), q.to(dev), *args, valid=valid.to(dev))
        return got_loss.clone(), got_grad.clone(), fn.per_image.clone(), fn.loss_f64.clone(), fn.valid_counts.clone()
    got = run(pred, target)
    got_loss, got_grad, got_per_image, got_f64, got_counts = got
    assert torch.equal(got_counts.cpu(), counts)
    assert torch.allclose(got_per_image.cpu(), per_image, rtol=GL.SUM_RTOL, atol=0.0)
    assert abs(got_f64.item() - loss.item()) <= GL.SUM_RTOL * abs(loss.item())
    assert abs(got_loss.item() - float(np.float32(loss.item()))) <= GL._ulp32(loss.item())
    GL._assert_grad(got_grad, grad, f"{shape} {kind} masked vs oracle")
    m = nd[:, None].expand(shape)
    under = got_grad.cpu()[m]
    assert bool((under == 0).all()) and not torch.signbit(under).any()
    for b in range(shape[0]):
        if counts[b] == 0:
            assert got_per_image[b].item() == 0.0 and not got_grad[b].any()
    assert all(bits_equal(a, b) for a, b in zip(got, run(pred, target)))  # repeatable
    # isolation: NaN, +-inf and 1e30 under the mask, in pred and in target
    junk_p = torch.where(m, _junk_like(pred, 1), pred)
    junk_q = torch.where(m, _junk_like(target, 2), target)
    assert all(bits_equal(a, b) for a, b in zip(got, run(junk_p, junk_q)))
    with torch.no_grad():
        assert bits_equal(fn(junk_p.to(dev), junk_q.to(dev), *args, valid=valid.to(dev)), got_loss)
    if not weighted:  # the scalar with an autograd function behind it
        q = pred.to(dev).requires_grad_()
        out = fn(q, target.to(dev), valid=valid.to(dev))
        (3.0 * out).backward()
        assert torch.equal(out.detach(), got_loss) and torch.equal(q.grad, got_grad * 3.0)


def test_loss_edge_cases(dev):
    """The image without a valid pixel is not binned and its ring untouched; a batch without a valid pixel has loss 0, zero
    gradients, empty bins; a t outside the table still makes the loss NaN and is counted."""
    from diffusionremotesensing_amd.losses import DiffusionLoss, LossBins
    pred, target, t, table, _ = GL._inputs(A)
    nd = _nodata(A)
    valid = (~nd).to(torch.uint8)[:, None].contiguous().to(dev)
    bins = LossBins(T, 4, dev)
    fn = DiffusionLoss("MSE", table.to(dev), bins)
    fn.loss_and_grad(pred.to(dev), target.to(dev), t.to(dev), valid=valid)
    want = GL.O.BinsOracle(T, 4)
    per_image = NO.masked_loss(pred, target, ~nd, "MSE")[0]
    want.update(per_image[[0, 2]], t[[0, 2]])  # image 1 has no valid pixel
    stats = bins.read_and_reset()
    assert stats["count"] == want.count and sum(stats["count"]) == 2 and stats["nonfinite"] == 0
    assert [len(r) for r in bins.ring()] == [len(r) for r in want.ring]
    none = torch.zeros_like(valid)
    loss, grad = fn.loss_and_grad(pred.to(dev), target.to(dev), t.to(dev), valid=none)
    assert loss.item() == 0.0 and fn.loss_f64.item() == 0.0 and not grad.any() and not torch.signbit(grad).any()
    assert fn.per_image.tolist() == [0.0] * 3 and fn.valid_counts.tolist() == [0] * 3
    assert sum(bins.read_and_reset()["count"]) == 0
    bad = t.clone()
    bad[0] = T
    loss, grad = fn.loss_and_grad(pred.to(dev), target.to(dev), bad.to(dev), valid=valid)
    assert math.isnan(loss.item()) and torch.isfinite(grad[2]).all()
    with pytest.raises(RuntimeError, match="1 timestep"):
        fn.check_faults()
    with pytest.raises(RuntimeError, match="uint8"):
        fn.loss_and_grad(pred.to(dev), target.to(dev), t.to(dev), valid=valid.float())
    with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
        fn.loss_and_grad(pred.to(dev).flatten(1), target.to(dev).flatten(1), t.to(dev), valid=valid)


@pytest.mark.parametrize("rule", ["nan", "value"])
@pytest.mark.parametrize("shape", [A, V1, V2, S], ids=str)
def test_metrics_vs_oracle(dev, shape, rule):
    """`metrics.image_quality(nodata=)` within test_gpu_metrics' TOL_* of the oracle, the counts exact; junk in sr under the mask
    and in the non-deciding bands of hr changes no output bit; two calls give the same bits."""
    from diffusionremotesensing_amd import hip_ops, metrics
    hr = _marked(shape, rule)
    g = torch.Generator().manual_seed(9)
    sr = (torch.nan_to_num(hr, nan=0.5) + 0.05 * torch.randn(shape, generator=g))
    nodata, value = _rule_value(rule), (None if rule == "nan" else VALUE)
    nd = _nodata(shape)
    C = shape[1]

    def run(s, h):
        q = metrics.image_quality(s.to(dev), h.to(dev), GM.MAG, nodata=nodata)
        return q, hip_ops.metrics_pointwise_nodata(s.to(dev), h.to(dev), nodata), hip_ops.ssim_nodata(s.to(dev), h.to(dev), nodata)
    got, sums, ss = run(sr, hr)
    want = NO.image_quality(sr, hr, GM.MAG, value)
    GM._assert_matches_oracle(got, want, (shape, rule))
    want_sums, want_ss = NO.pointwise_sums(sr, hr, value), NO.ssim(sr, hr, value)
    assert torch.equal(sums[:, 2 * C + 1:].cpu(), want_sums[:, 2 * C + 1:]) and torch.equal(ss[:, 1].cpu(), want_ss[:, 1])
    # (torch divides by a scalar on the device with a product by its inverse: one more rounding than the quotient)
    assert torch.allclose(got["valid_fraction"].cpu(), (~nd).sum(dim=(1, 2)).double() / (shape[2] * shape[3]), rtol=2.0 ** -51, atol=0)
    for b in range(shape[0]):
        if nd[b].all():  # no valid pixel: no score
            assert all(math.isnan(got[k][b].item()) for k in got if k != "valid_fraction")
    if shape == S:  # one window: any no-data pixel leaves none
        assert [math.isnan(v) for v in ss[:, 0].tolist()] == [False, True, True, True, True] and ss[:, 1].tolist() == [1, 0, 0, 0, 0]
    again = run(sr, hr)
    flat = lambda r: list(r[0].values()) + [r[1], r[2]]  # noqa: E731
    assert all(bits_equal(a, b) for a, b in zip(flat((got, sums, ss)), flat(again)))
    # isolation
    m = nd[:, None].expand(shape)
    junk_sr = torch.where(m, _junk_like(sr, 3), sr)
    free = m & ~torch.isnan(hr) if rule == "nan" else torch.zeros_like(m)  # hr's bands that do not decide the mask
    junk = _junk_like(hr, 4)
    junk_hr = torch.where(free, torch.where(torch.isnan(junk), torch.full_like(junk, -1e30), junk), hr)  # (a NaN would decide too)
    assert all(bits_equal(a, b) for a, b in zip(flat((got, sums, ss)), flat(run(junk_sr, junk_hr))))
    for name, fn in (("psnr", metrics.psnr), ("ssim", metrics.ssim), ("ergas", lambda *a, **k: metrics.ergas(*a[:2], GM.MAG, **k))):
        assert bits_equal(fn(sr.to(dev), hr.to(dev), nodata=nodata), got[name]), name
    if C >= 2:
        assert bits_equal(metrics.sam(sr.to(dev), hr.to(dev), nodata=nodata), got["sam"])


def test_value_rule_keeps_nan_pixels_and_mixed_bands(dev):
    """Under the value rule a NaN pixel is no-data too, a pixel holding the value in some bands only is data, and hr's other
    bands at a NaN-decided pixel may hold anything."""
    from diffusionremotesensing_amd import hip_ops
    g = torch.Generator().manual_seed(11)
    hr = torch.rand((1, 3, 12, 12), generator=g) * 0.9 + 0.05
    sr = hr + 0.01
    hr[0, 1, 3, 4] = math.nan
    hr[0, :, 5, 5] = VALUE
    hr[0, 0, 7, 7] = VALUE
    want = NO.pointwise_sums(sr, hr, VALUE)
    assert want[0, -1].item() == 144 - 2
    got = hip_ops.metrics_pointwise_nodata(sr.to(dev), hr.to(dev), VALUE)
    assert got[0, -1].item() == 142 and torch.allclose(got.cpu(), want, rtol=1e-5)
    other = hr.clone()
    other[0, 0, 3, 4], other[0, 2, 3, 4] = math.inf, 1e30
    assert bits_equal(hip_ops.metrics_pointwise_nodata(sr.to(dev), other.to(dev), VALUE), got)
    assert bits_equal(hip_ops.ssim_nodata(sr.to(dev), other.to(dev), VALUE), hip_ops.ssim_nodata(sr.to(dev), hr.to(dev), VALUE))


def test_ssim_pivot_avoids_no_data(dev):
    """A no-data pixel at the tile's middle - where the unmasked kernel takes its pivot - with junk in both images there: the
    positions away from it are scored, on bright flat terrain where a pivot of zero would cost the moments their digits."""
    from diffusionremotesensing_amd import hip_ops
    shape = (1, 2, 40, 44)
    sr, hr = GM._pair(shape, "bright_flat")
    hr[0, :, 21, 21] = math.nan
    sr[0, :, 21, 21] = math.inf
    got = hip_ops.ssim_nodata(sr.to(dev), hr.to(dev), True).cpu()
    want = NO.ssim(sr, hr)
    assert got[0, 1] == want[0, 1] > 0 and abs(got[0, 0] - want[0, 0]) <= GM.TOL_SSIM


# ---- the mask through the feed ---------------------------------------------------------------------------------------------
def test_mask_survives_the_crop_under_every_symmetry(dev):
    """`crop_d4_pairs` carries the NaN marker through all 8 dihedral codes: the `valid` of the feed's batch is the oracle's mask
    of the transformed window."""
    from diffusionremotesensing_amd import hip_ops
    from diffusionremotesensing_amd.augment import crop_d4_pairs, upload_items
    g = torch.Generator().manual_seed(13)
    L, H, W, size = 2, 14, 17, 9
    sar, ndvi = torch.rand((L, 2, H, W), generator=g) * 2 - 1, torch.rand((L, 2, H, W), generator=g) * 2 - 1
    hole = torch.rand((L, H, W), generator=g) < 0.2
    ndvi[:, 0][hole] = math.nan  # band 0 carries the marker, band 1 keeps its values
    items = np.array([[i % L, 1 + i % 3, 2 + i % 5, code] for i, code in enumerate(range(8))], dtype=np.int32)
    _, batch = crop_d4_pairs(sar.to(dev), ndvi.to(dev), upload_items(items, dev), size)

    def d4(w, code):
        if code & 4:
            w = w.swapaxes(-1, -2)
        if code & 1:
            w = w.flip(-1)
        if code & 2:
            w = w.flip(-2)
        return w
    windows = torch.stack([d4(ndvi[s, :, y:y + size, x:x + size], code) for s, y, x, code in items.tolist()])
    want = NO.valid_mask((windows + 1) * 0.5)
    assert 0 < int((~want).sum()) < want.numel() and torch.equal(want, ~d4_holes(hole, items, size, d4))
    eps = torch.randn(batch.shape, generator=g).to(dev)
    t = torch.randint(1, T, (8,), generator=g).to(dev)
    _, target, valid = hip_ops.noise_target_nodata(batch, eps, t, _schedule().to(dev), "x0")
    assert torch.equal(valid[:, 0].bool().cpu(), want)
    assert torch.equal(target.cpu()[want[:, None].expand_as(target)], ((windows + 1) * 0.5)[want[:, None].expand_as(target)])


def d4_holes(hole, items, size, d4):
    return torch.stack([d4(hole[s, y:y + size, x:x + size], code) for s, y, x, code in items.tolist()])


# ---- end to end ------------------------------------------------------------------------------------------------------------
SIZE, PAIRS = 32, 8


def _write_sar_pairs(root, n, seed, scramble):
    """n (SAR, NDVI) .pt pairs of 32 x 32, two bands each; in every NDVI image a stripe of 11 columns - a third of its pixels -
    is NaN in band 0, and band 1 there holds seeded values, or junk with `scramble`."""
    g = torch.Generator().manual_seed(seed)
    for sub in ("sar", "opt"):
        os.makedirs(os.path.join(root, sub))
    holes = torch.zeros(n, SIZE, SIZE, dtype=torch.bool)
    for i in range(n):
        sar, ndvi = torch.rand((2, SIZE, SIZE), generator=g) * 2 - 1, torch.rand((2, SIZE, SIZE), generator=g) * 1.6 - 0.8
        x = (5 * i) % 22
        holes[i, :, x:x + 11] = True
        ndvi[0, :, x:x + 11] = math.nan
        if scramble:
            junk = _junk_like(ndvi[1, :, x:x + 11], seed + i)
            ndvi[1, :, x:x + 11] = torch.where(torch.isnan(junk), torch.full_like(junk, -3e30), junk)
        torch.save(sar, os.path.join(root, "sar", f"{i:02d}.pt"))
        torch.save(ndvi, os.path.join(root, "opt", f"{i:02d}.pt"))
    return holes


def _train_sar(dev, root, nodata, epochs=2, shadow_root=None):
    """Two epochs over the 8 pairs in batches of 4 (files read as they are: band 0's NaN is the marker, band 1 keeps what the
    files hold under it): (the loss of every step, the trained parameters, the Diffusion, the model, the validation feed).
    With `shadow_root` - a folder of the same items - every step is first derived twice from the weights as they stand, under
    the step's own draw of t and eps: from the run's batch and from the shadow folder's batch of the same items.  x_t, target,
    mask, prediction, loss, d loss / d prediction and the per-image figures must agree bit for bit between the two, and the
    derived loss with the loss the real step then returns; the number of steps compared comes back as a sixth value."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd import train_diffusion_SAR_TO_NDVI as SN
    from diffusionremotesensing_amd.feeds import DeviceSarNdviFeed, load_sar_ndvi_folder
    from diffusionremotesensing_amd.losses import DiffusionLoss
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    sar, ndvi = load_sar_ndvi_folder(root)
    feed = DeviceSarNdviFeed(sar.to(dev), ndvi.to(dev), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(1))
    val = DeviceSarNdviFeed(sar[:4].to(dev), ndvi[:4].to(dev), batch_size=4, shuffle=False)
    shadow = None
    if shadow_root is not None:
        shadow_sar, shadow_ndvi = load_sar_ndvi_folder(shadow_root)
        assert torch.equal(shadow_sar, sar) and not bits_equal(shadow_ndvi, ndvi)  # the same items, other values under the mask
        shadow = DeviceSarNdviFeed(shadow_sar.to(dev), shadow_ndvi.to(dev), batch_size=4, shuffle=True,
                                   generator=torch.Generator().manual_seed(1))  # (the same order, epoch after epoch)
    model = Residual_Attention_UNet_SAR_TO_NDVI(2, 2, dev)
    model.load_state_dict(synthetic.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev)
    d = SN.Diffusion("cosine", model, os.path.join(root, "weights", "snapshot.pt"), noise_steps=20, device=dev, image_size=SIZE)
    os.makedirs(os.path.join(root, "weights"), exist_ok=True)
    d.nodata = nodata
    losses, step, state = [], d.train_step, {"iter": None, "compared": 0}

    def derive(net, sar_b, ndvi_b):
        t = d.sample_timesteps(ndvi_b.shape[0]).to(dev)
        x_t, target, valid = d._noised_target(ndvi_b, t)
        pred = net(x_t, t, sar_b)  # in train mode, as the step runs it
        fn = DiffusionLoss("MSE")
        loss, grad = fn.loss_and_grad(pred, target, t, valid=valid)
        return x_t, target, valid, pred.detach(), loss.clone(), grad, fn.per_image, fn.valid_counts

    def recording(net, optimizer, loss_function, sar_b, ndvi_b, *a, **k):
        derived = None
        if shadow is not None:
            if len(losses) % len(feed) == 0:
                state["iter"] = iter(shadow)
            shadow_b = next(state["iter"])
            assert torch.equal(shadow_b[0], sar_b) and not bits_equal(shadow_b[1], ndvi_b)
            rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
            outs = []
            for pair in ((sar_b, ndvi_b), shadow_b):
                torch.set_rng_state(rng[0])
                torch.cuda.set_rng_state(rng[1], dev)
                outs.append(derive(net, *pair))
            for x, y in zip(*outs):
                assert bits_equal(x, y), f"step {len(losses)}"
            assert all(torch.isfinite(v.double()).all() for v in outs[1])
            derived = outs[0][4]
            torch.set_rng_state(rng[0])
            torch.cuda.set_rng_state(rng[1], dev)
        losses.append(step(net, optimizer, loss_function, sar_b, ndvi_b, *a, **k))
        if derived is not None:
            assert bits_equal(losses[-1].detach(), derived), f"step {len(losses) - 1}: the derivation is not the step's"
            state["compared"] += 1
        return losses[-1]
    d.train_step = recording
    torch.manual_seed(0)
    d.train(lr=1e-3, epochs=epochs, check_preds_epoch=1, train_loader=feed, val_loader=val, patience=5, loss="MSE", verbose=False)
    return [v.item() for v in losses], [p.detach().clone() for p in model.parameters()], d, model, val, state["compared"]


def test_sar_training_and_evaluate_with_nodata(dev, tmp_path):
    """Two epochs of `Diffusion_SAR_TO_NDVI` on 8 pairs with a third of the NDVI pixels marked: on the files as written, and on
    the same files with junk (NaN, +-inf, 1e30) in the band under the mask that does not carry the marker.
    That the values under the mask do not matter is held bit for bit at every one of the four steps, from shared weights
    (`_train_sar(shadow_root=)`): x_t, target, mask, prediction, loss and d loss / d prediction of the junk batch are those of
    the clean batch, and the derived loss is the one the step returns.  The run on the junk files itself must stay finite in
    every loss and parameter, and its first loss - the one no update precedes - has the clean run's bits.
    Two whole runs are not compared bit for bit beyond that, because two runs on the SAME files do not agree either: the weight
    gradients are reduced with float atomics (tests/test_gpu_guard.py, _ATOMICS), and Adam turns the rounding noise of a
    gradient that is analytically zero (a bias in front of a BatchNorm) into a step of +-lr.  Measured on MI355X, same files
    twice: 168 of 176 parameter tensors differ, by up to 2.3e-3 = 2 lr after four steps; the four losses agreed to the bit in
    one session and the fourth was 1 ulp apart in another."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.losses import DiffusionLoss
    from diffusionremotesensing_amd.optim import FusedAdam
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    root_a, root_b = str(tmp_path / "a"), str(tmp_path / "b")
    holes = _write_sar_pairs(root_a, PAIRS, 7, scramble=False)
    _write_sar_pairs(root_b, PAIRS, 7, scramble=True)
    assert abs(holes.float().mean().item() - 1 / 3) < 0.02
    start = synthetic.seeded_state_dict(Residual_Attention_UNet_SAR_TO_NDVI(2, 2, dev).state_dict(), 0)
    losses, params, d, model, val, compared = _train_sar(dev, root_a, True, shadow_root=root_b)
    assert compared == len(losses) == 4 and all(math.isfinite(v) for v in losses), losses
    assert isinstance(d.train_state.loss_function, DiffusionLoss) and d.train_state.loss_function.valid_counts is not None
    assert all(torch.isfinite(p).all() for p in params)
    assert any(not torch.equal(p.cpu(), start[name]) for (name, _), p in zip(model.named_parameters(), params))
    # the run on the junk files: finite throughout, and the clean run's bits where no irreproducible update comes first
    losses_b, params_b, _, _, _, _ = _train_sar(dev, root_b, True)
    differ = [(p - q).abs().max().item() for p, q in zip(params, params_b) if not bits_equal(p, q)]
    print(f"run on the junk files: losses {losses_b} against {losses}; {len(differ)} of {len(params)} parameter tensors differ, "
          f"max |diff| {max(differ, default=0.0):.3e}")
    assert len(losses_b) == 4 and all(math.isfinite(v) for v in losses_b) and all(torch.isfinite(p).all() for p in params_b)
    assert losses_b[0] == losses[0]
    scores = d.evaluate(model, val, sampling_steps=4, nodata=True)
    assert scores["n"] == 4 and set(scores["model"]) == {"psnr", "ssim", "sam", "valid_fraction"}
    assert all(math.isfinite(v) for v in scores["model"].values()), scores["model"]
    assert scores["per_image"]["model"]["valid_fraction"] == [1 - 11 / 32] * 4
    with pytest.raises(ValueError, match="cannot be combined"):
        d.evaluate(model, val, sampling_steps=4, nodata=True, ensemble=2)
    # today's behaviour, pinned as the contrast: the same data without the setting poisons the loss of the whole batch
    d.nodata = None
    model.train()  # (the validation epoch left it in eval mode)
    sar, ndvi = next(iter(val))
    loss = type(d).train_step(d, model, FusedAdam(model.parameters(), lr=1e-3), torch.nn.MSELoss(), sar, ndvi)
    assert math.isnan(loss.item())
