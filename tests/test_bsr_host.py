"""Host side of the blind degradation (diffusionremotesensing_amd/bsr.py): the recipe, and the float64 / integer oracle the GPU
tests compare against (tests/bsr_oracle.py) checked against scipy and Pillow.  No GPU."""
import io
import math

import numpy as np
import pytest

import bsr_oracle as BO
from diffusionremotesensing_amd import bsr


def _recipes(kind, c=3, count=40, **kw):
    rng = np.random.default_rng(5)
    return [bsr.draw_recipe(rng, 4, c, 64, 64, 2, kind, **kw) for _ in range(count)]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a, b)
    return a == b


def test_recipe_is_deterministic_under_a_seed():
    for kind in bsr.KINDS:
        a = [bsr.draw_recipe(np.random.default_rng(9), 3, 3, 64, 48, 4, kind) for _ in range(2)]
        assert _same(a[0], a[1])
        assert not _same(a[0], bsr.draw_recipe(np.random.default_rng(10), 3, 3, 64, 48, 4, kind))


@pytest.mark.parametrize("sf", [2, 4])
def test_every_parameter_is_inside_the_reference_range(sf):
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(60):
        r = bsr.draw_recipe(rng, 5, 3, 64, 64, sf, "plus")
        assert sorted(r["order"]) == list(range(13)) and r["sharpen"]
        h = w = 64
        for op in r["ops"]:
            seen.add(op["op"])
            if op["op"] == "blur":
                assert op["kernels"].shape[0] == 5 and op["kernels"].shape[1] == op["ksize"].max() <= bsr.MAX_KSIZE
                assert set(op["ksize"].tolist()) <= set(range(7, 26, 2))      # 2 randint(2, 11) + 3
                assert (0 <= op["theta"]).all() and (op["theta"] < math.pi).all()
                assert (0 < op["l1"]).all() and (op["l1"] < 4 + sf).all() and (0 < op["l2"]).all() and (op["l2"] < 4 + sf).all()
                assert (0 < op["sigma"]).all() and (op["sigma"] < 2 + 0.2 * sf).all()
                assert (op["kernels"] >= 0).all() and np.allclose(op["kernels"].sum(axis=(1, 2)), 1, atol=1e-5)
                for i, ks in enumerate(op["ksize"]):  # the table is zero outside the image's centred kernel
                    o = (op["kernels"].shape[1] - ks) // 2
                    inner = op["kernels"][i, o:o + ks, o:o + ks]
                    assert inner.sum() == pytest.approx(op["kernels"][i].sum())
            elif op["op"] == "resize" and op["slot"] != "final":
                assert op["mode"] in (1, 2, 3) and (0.5 / sf <= op["factor"] <= 2)
                assert (op["out_h"], op["out_w"]) == (max(int(op["factor"] * h), 1), max(int(op["factor"] * w), 1))
                h, w = op["out_h"], op["out_w"]
            elif op["op"] in ("noise", "speckle"):
                assert ((2 <= op["level"]) & (op["level"] <= 25)).all() and set(op["branch"].tolist()) <= {0, 1, 2}
                assert op["on"].all() or op["op"] == "speckle"
                for A in op["A"]:  # A A^T is |L^2 U^T D U|: symmetric, entries below L^2
                    cov = A @ A.T
                    assert np.allclose(cov, cov.T) and (np.abs(cov) <= (25 / 255) ** 2 + 1e-12).all()
            elif op["op"] == "poisson":
                assert ((100 <= op["vals"]) & (op["vals"] <= 10000)).all()
            elif op["op"] == "jpeg":
                assert ((30 <= op["quality"]) & (op["quality"] <= 95)).all() and op["quality"].dtype == np.int32
    assert seen == {"blur", "resize", "noise", "speckle", "poisson", "jpeg", "isp"}


def test_order_rules_and_the_final_ops():
    for r in _recipes("plus", shuffle_prob=0.0):
        assert not r["shuffled"]
        assert [r["order"][i] for i in (0, 1, 6, 7, 8)] == [0, 1, 6, 7, 8]
        assert sorted(r["order"][2:6]) == [2, 3, 4, 5] and sorted(r["order"][9:13]) == [9, 10, 11, 12]
    assert any(r["order"] != list(range(13)) for r in _recipes("plus", shuffle_prob=0.0))
    assert any(r["order"][0] != 0 for r in _recipes("plus", shuffle_prob=1.0))
    for kind in bsr.KINDS:
        for r in _recipes(kind):
            names = [(op["op"], op["slot"]) for op in r["ops"]]
            final = [("resize", "final"), ("jpeg", "final")] if kind == "plus" else [("resize", "final")]
            assert names[-len(final):] == final
            assert (r["ops"][-len(final)]["out_h"], r["ops"][-len(final)]["out_w"]) == (32, 32)
            assert [op["slot"] for op in r["ops"][:-len(final)]] == r["order"]
            if kind == "soft":
                assert not r["sharpen"] and sorted(r["order"]) == [0, 1, 2] and all(op["op"] != "jpeg" for op in r["ops"])


def test_thirteen_bands_hold_no_jpeg_and_no_correlated_or_gray_branch():
    for r in _recipes("plus", c=13):
        for op in r["ops"]:
            assert op["op"] != "jpeg"
            if op["op"] in ("noise", "speckle"):
                assert (op["branch"] != bsr.BRANCH_CORR).all()
            if op["op"] == "poisson":
                assert not op["gray"].any()
    assert any((op["op"] == "noise" and (op["branch"] == bsr.BRANCH_CORR).any()) for r in _recipes("plus") for op in r["ops"])


def test_geometry_is_shared_and_the_rest_is_per_image():
    for r in _recipes("plus"):
        for op in r["ops"]:
            if op["op"] == "resize":
                assert all(np.ndim(op[k]) == 0 for k in ("mode", "out_h", "out_w"))
            for k in ("ksize", "level", "vals", "quality", "on", "branch"):
                if k in op:
                    assert np.shape(op[k]) == (4,)
    blurs = [op for r in _recipes("plus") for op in r["ops"] if op["op"] == "blur"]
    assert any(len(set(op["ksize"].tolist())) > 1 for op in blurs)


def test_kernel_table_holds_the_reference_kernels():
    """The batched closed form against the per-image restatements of `anisotropic_Gaussian` / `fspecial('gaussian')`, and the
    anisotropic one against scipy's density, as the reference evaluates it."""
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(8)
    n = 12
    ksize, aniso = 2 * rng.integers(2, 12, n) + 3, rng.random(n) < 0.5
    theta, l1, l2, sigma = rng.random(n) * math.pi, 6 * rng.random(n) + 1e-3, 6 * rng.random(n) + 1e-3, 2.4 * rng.random(n) + 1e-3
    sigma[0], aniso[0] = 1e-3, False  # a delta
    table = bsr.kernel_table(ksize, aniso, theta, l1, l2, sigma)
    K = int(ksize.max())
    assert table.shape == (n, K, K) and table.dtype == np.float32
    for i in range(n):
        ks, o = int(ksize[i]), (K - int(ksize[i])) // 2
        want = bsr.anisotropic_gaussian(ks, theta[i], l1[i], l2[i]) if aniso[i] else bsr.isotropic_gaussian(ks, sigma[i])
        full = np.zeros((K, K))
        full[o:o + ks, o:o + ks] = want
        assert np.abs(table[i] - full).max() <= 1e-7
    assert table[0, K // 2, K // 2] == 1
    v = np.array([math.cos(0.7), math.sin(0.7)])
    V = np.array([[v[0], v[1]], [v[1], -v[0]]])
    cov = V @ np.diag([3.0, 0.8]) @ np.linalg.inv(V)
    ref = np.array([[multivariate_normal.pdf([x - 4, y - 4], mean=[0, 0], cov=cov) for x in range(9)] for y in range(9)])
    assert np.abs(bsr.anisotropic_gaussian(9, 0.7, 3.0, 0.8) - ref / ref.sum()).max() <= 1e-12


def test_usm_taps_follow_the_sigma_rule():
    t = bsr.usm_taps()
    assert t.shape == (51,) and t.dtype == np.float32
    assert np.abs(t - BO.gaussian_taps(51)).max() <= 2.0 ** -24 * t.max()
    assert t[25] / t[17] == pytest.approx(math.exp(0.5), rel=1e-6)  # sigma 8: one sigma out


# ---- oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,k", [((5, 7), 25), ((1, 1), 7), ((33, 47), 15), ((12, 30), 3)])
def test_oracle_blur_is_scipy_convolve_mirror(shape, k):
    from scipy.ndimage import convolve
    rng = np.random.default_rng(k + shape[0])
    img, ker = rng.random(shape), rng.random((k, k))
    ker /= ker.sum()
    want = convolve(img, ker, mode="mirror")
    assert np.abs(BO.blur_plane(img, ker) - want).max() <= 1e-13
    taps = rng.random(k)
    assert np.abs(BO.blur_sep(img[None, None], taps)[0, 0] - convolve(img, np.outer(taps, taps), mode="mirror")).max() <= 1e-12


def test_oracle_resize_definitions():
    rng = np.random.default_rng(1)
    x = rng.random((1, 2, 8, 8))
    for mode in (1, 2, 3):
        assert np.array_equal(BO.resize(x, 8, 8, mode), x)
        for n_in, n_out in ((33, 16), (33, 50), (47, 1), (8, 8)):
            assert np.allclose(BO.axis_matrix(n_in, n_out, mode).sum(axis=1), 1, atol=1e-12)
    assert np.allclose(BO.resize(x, 4, 4, 3), x.reshape(1, 2, 4, 2, 4, 2).mean(axis=(3, 5)))       # area by 2: the 2 x 2 mean
    assert np.allclose(BO.resize(x, 1, 1, 3)[..., 0, 0], x.mean(axis=(2, 3)))
    assert np.allclose(BO.resize(x, 4, 4, 1), x.reshape(1, 2, 4, 2, 4, 2).mean(axis=(3, 5)))       # bilinear by 2 lands between
    assert np.allclose(BO.cubic_weights(0.5), [-0.09375, 0.59375, 0.59375, -0.09375])  # a = -0.75 half way between samples
    assert np.allclose(BO.cubic_weights(0.0), [0, 1, 0, 0]) and np.allclose(BO.cubic_weights(0.25).sum(), 1)
    assert np.allclose(BO.axis_matrix(8, 4, 2)[1], [0, -0.09375, 0.59375, 0.59375, -0.09375, 0, 0, 0])  # no antialiasing: 4 taps


def test_dct_literal_is_the_rounded_cosine_matrix():
    assert np.array_equal(BO.DCT, BO.dct_matrix())
    assert np.abs(BO.DCT).sum(axis=1).max() == 46344  # the int32 bound of DESIGN.md section 19
    assert np.abs(BO.DCT @ BO.DCT.T - np.eye(8) * 2 ** 28).max() <= 2 ** 28 * 2e-4  # orthonormal to 14 bits


def _textured(h, w, seed):
    """A seeded RGB image with edges, gradients and fine texture."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 3))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.05, 0.6, 2).tolist() + [rng.uniform(0, 6)]
        img[..., c] = 128 + 60 * np.sin(fy * y + fx * x + ph) + 40 * ((x // 5 + y // 7 + c) % 2) + rng.normal(0, 12, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _pillow_jpeg(rgb, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=2)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"), dtype=np.int64)


QUALITIES = (30, 50, 70, 90)


@pytest.mark.parametrize("size", [(16, 16), (32, 48), (48, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_jpeg_vs_pillow(size):
    """Pillow (libjpeg-turbo) stands in for cv2's codec; 4:2:0, sides that are multiples of 16.  At every tested quality the mean
    absolute difference from Pillow is at most 1/4 of the mean absolute difference between Pillow at that quality and Pillow at the
    nearest other tested quality (for 50 and 70, the nearer-looking of the two neighbours: the smaller difference).
    Measured with the integer DCT, the ratio at q = 30 / 50 / 70 / 90: 16x16 0.005 / 0.047 / 0.033 / 0.086, 32x48 0.051 / 0.060 /
    0.067 / 0.082, 48x64 0.006 / 0.013 / 0.040 / 0.079."""
    rgb = _textured(size[0], size[1], 17 + size[1])
    pil = {q: _pillow_jpeg(rgb, q) for q in QUALITIES}
    for i, q in enumerate(QUALITIES):
        mine = BO.jpeg_u8(rgb, q).astype(np.int64)
        assert mine.shape == rgb.shape
        d = np.abs(mine - pil[q]).mean()
        step = min(np.abs(pil[q] - pil[o]).mean() for o in QUALITIES[max(i - 1, 0):i + 2] if o != q)
        print(f"jpeg {size} q={q}: |oracle - pillow| {d:.4f}, |pillow(q) - pillow(neighbour)| {step:.4f}, ratio {d / step:.3f}")
        assert step > 0.5 and d <= 0.25 * step, (size, q, d, step)


def test_oracle_jpeg_rules():
    """A flat gray image survives every quality; quality 100 is all-ones tables; a lower quality moves further from the input."""
    flat = np.full((16, 32, 3), 77, dtype=np.uint8)
    for q in (30, 95):
        assert np.array_equal(BO.jpeg_u8(flat, q), flat)
    assert (BO.quant_table(0, 100) == 1).all() and BO.quant_table(0, 50)[0, 0] == 16 and BO.quant_table(1, 25)[7, 7] == 198
    rgb = _textured(32, 32, 3)
    err = [np.abs(BO.jpeg_u8(rgb, q).astype(int) - rgb).mean() for q in (30, 60, 95)]
    assert err[0] > err[1] > err[2]
    x = rgb.transpose(2, 0, 1)[None].astype(np.float32) / np.float32(255)
    assert np.array_equal(BO.jpeg(x, [60])[0], BO.jpeg_u8(rgb, 60).transpose(2, 0, 1).astype(np.float32) / np.float32(255))
    odd = BO.jpeg_u8(rgb[:21, :27], 80)  # the edge rule: as the image padded by its edge pixels, cropped
    padded = rgb[np.minimum(np.arange(32), 20)][:, np.minimum(np.arange(32), 26)]
    assert np.array_equal(odd, BO.jpeg_u8(padded, 80)[:21, :27])
