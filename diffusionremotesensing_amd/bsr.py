"""Blind (BSRGAN-plus) degradation on the device: the `Degradation_type="BSRGAN"` feed of the super-resolution trainer.

The reference runs `degradation_bsrgan_plus` (degradation_from_BSRGAN.py:684-768; `soft_degradation_bsrgan` :770-816) with numpy,
cv2 and scipy on the host, once per image at start-up, and keeps `num_crops` frozen copies.  Here every batch gets a FRESH random
degradation on the device, from the uint8 HR cache `DeviceSuperresFeed` keeps there (Real-ESRGAN's form of the same pipeline):

    recipe   `draw_recipe` (host, numpy): the reference's slots, ordering rules and distributions (:498-581) from one seeded
             `numpy.random.Generator` - its distributions, not its stream, which cannot be reproduced (`np.random.poisson(img *
             vals)` consumes it depending on the pixels).  The slot order and every resize factor and mode are drawn ONCE PER
             BATCH, so every intermediate tensor stays dense (N, C, h', w'); blur kernel, noise branch / level / covariance factor,
             Poisson and speckle on / off and the JPEG quality are drawn PER IMAGE.  A per-image op that is off leaves its image
             untouched.
    ops      `blur`, `sharpen`, `resize`, `noise_`, `jpeg`: HIP kernels (csrc/bsr_degrade.hip, definitions in include/drs_hip.h and
             DESIGN.md section 19), no CPU path.  Normal and Poisson draws come from torch on the device, from the feed's
             `torch.Generator`; a batch's per-image parameters travel in one upload.
    feed     `DeviceBSRFeed`: (lr, hr) float32 batches in [0, 1]; HR is the cached image_size x image_size image (USM-sharpened
             for kind "plus", as the reference's `hq` is), LR is image_size // m on a side and lies on the k / 255 grid like the
             reference's stored dataset.

`random_crop` and `num_crops` of the reference's dataset are the feed's `crop_size` / `num_crops` arguments (augment.py: fresh
windows per batch, cut on the device); without them the cache already holds the training images.  Dropped from the reference: its
BSRGAN-mode meaning of `image_size` (the LR size).  With c != 3 bands JPEG is skipped, the correlated-noise branch falls to
per-band noise and the gray Poisson branch to the per-band one: those need 3 bands in the reference as well.  The ISP slots are
no-ops (`isp_model` is always None there).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

KINDS = ("plus", "soft")
BILINEAR, BICUBIC, AREA = 1, 2, 3  # cv2's interpolation flags 1 / 2 / 3, which the reference draws from
MAX_KSIZE = 25
NOISE_OFF, NOISE_ADD, NOISE_SPECKLE, NOISE_POISSON, NOISE_POISSON_GRAY = 0, 1, 2, 3, 4
BRANCH_BAND, BRANCH_GRAY, BRANCH_CORR = 0, 1, 2
USM_KSIZE, USM_WEIGHT, USM_THRESHOLD = 51, 0.5, 10.0  # add_sharpening(img, weight=0.5, radius=50, threshold=10): radius 50 -> 51
# slots of degradation_bsrgan_plus (:721-757) and of soft_degradation_bsrgan (:800-808)
PLUS_SLOTS = ("blur", "resize", "noise", "poisson", "speckle", "isp", "jpeg", "blur", "resize", "noise", "poisson", "speckle", "isp")
SOFT_SLOTS = ("blur", "resize", "noise")


# ---------------------------------------------------------------------------------------------
# recipe (host)
# ---------------------------------------------------------------------------------------------
def usm_taps(k=USM_KSIZE):
    """The 1-D Gaussian of `cv2.GaussianBlur(img, (k, k), 0)`: sigma = 0.3 ((k - 1) / 2 - 1) + 0.8 (8 for k = 51), normalised."""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    x = np.arange(k, dtype=np.float64) - (k - 1) / 2
    g = np.exp(-x * x / (2 * sigma * sigma))
    return (g / g.sum()).astype(np.float32)


def anisotropic_gaussian(ksize, theta, l1, l2):
    """`anisotropic_Gaussian` / `gm_blur_kernel` of the reference (:228-260): the density of N(0, Sigma) at the integer offsets
    (cx, cy) from the centre, Sigma = V diag(l1, l2) V^-1 with V's first column (cos theta, sin theta), normalised to sum 1."""
    v0, v1 = math.cos(theta), math.sin(theta)
    V = np.array([[v0, v1], [v1, -v0]])
    inv = np.linalg.inv(V @ np.diag([l1, l2]) @ np.linalg.inv(V))
    r = ksize // 2
    cy, cx = np.meshgrid(np.arange(-r, r + 1.0), np.arange(-r, r + 1.0), indexing="ij")
    k = np.exp(-0.5 * (inv[0, 0] * cx * cx + (inv[0, 1] + inv[1, 0]) * cx * cy + inv[1, 1] * cy * cy))
    return k / k.sum()


def isotropic_gaussian(ksize, sigma):
    """`fspecial('gaussian', ksize, sigma)` of the reference (:351-362)."""
    r = ksize // 2
    y, x = np.meshgrid(np.arange(-r, r + 1.0), np.arange(-r, r + 1.0), indexing="ij")
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(float).eps * h.max()] = 0
    return h / h.sum()


def kernel_table(ksize, aniso, theta, l1, l2, sigma):
    """The (n, K, K) float32 table of a batch's blur kernels, K = max(ksize), image i's `anisotropic_gaussian(ksize[i], theta[i],
    l1[i], l2[i])` or `isotropic_gaussian(ksize[i], sigma[i])` centred in its plane and zeros around it - all images at once (V is
    its own inverse, so Sigma^-1 = V diag(1 / l1, 1 / l2) V in closed form): a batch's recipe is drawn per training step."""
    n, K = len(ksize), int(np.max(ksize))
    t = np.arange(K, dtype=np.float64) - K // 2
    cy, cx = t[None, :, None], t[None, None, :]
    col = lambda a: np.asarray(a, dtype=np.float64).reshape(n, 1, 1)  # noqa: E731
    v0, v1 = np.cos(col(theta)), np.sin(col(theta))
    a = v0 * v0 / col(l1) + v1 * v1 / col(l2)
    b = v0 * v1 * (1 / col(l1) - 1 / col(l2))
    c = v1 * v1 / col(l1) + v0 * v0 / col(l2)
    ka = np.exp(-0.5 * (a * cx * cx + 2 * b * cx * cy + c * cy * cy))
    ki = np.exp(-(cx * cx + cy * cy) / (2 * col(sigma) ** 2))
    r = col(ksize) // 2
    inside = (np.abs(cx) <= r) & (np.abs(cy) <= r)
    ki = np.where(inside, ki, 0.0)
    ki[ki < np.finfo(float).eps * ki.max(axis=(1, 2), keepdims=True)] = 0
    k = np.where(col(aniso).astype(bool), np.where(inside, ka, 0.0), ki)
    return (k / k.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


def _draw_blur(rng, n, sf):
    """`add_blur` (:498-509) for n images: anisotropic with probability 1/2 (eigenvalues in [0, 4 + sf), angle in [0, pi)),
    else isotropic (sigma in [0, 2 + 0.2 sf)); ksize = 2 randint(2, 11) + 3.  Widths are floored at 1e-3 (the reference's own
    draws hit 0 with probability 0, where scipy raises)."""
    aniso = rng.random(n) < 0.5
    ksize = (2 * rng.integers(2, 12, n) + 3).astype(np.int32)
    theta = rng.random(n) * math.pi
    l1 = np.maximum((4.0 + sf) * rng.random(n), 1e-3)
    l2 = np.maximum((4.0 + sf) * rng.random(n), 1e-3)
    sigma = np.maximum((2.0 + 0.2 * sf) * rng.random(n), 1e-3)
    kernels = kernel_table(ksize, aniso, theta, l1, l2, sigma)
    return {"op": "blur", "aniso": aniso, "ksize": ksize, "theta": theta, "l1": l1, "l2": l2, "sigma": sigma, "kernels": kernels}


def _draw_resize(rng, sf, h, w):
    """`add_resize` (:512-523), once for the batch: up by U(1, 2) with probability 0.2, down by U(0.5 / sf, 1) with 0.7, else
    as is; the mode one of cv2's 1 / 2 / 3."""
    rnum = rng.random()
    if rnum > 0.8:
        sf1 = rng.uniform(1, 2)
    elif rnum < 0.7:
        sf1 = rng.uniform(0.5 / sf, 1)
    else:
        sf1 = 1.0
    return {"op": "resize", "factor": float(sf1), "mode": int(rng.integers(1, 4)), "out_h": max(int(sf1 * h), 1),
            "out_w": max(int(sf1 * w), 1)}


def covariance_factor(rng, level2=25):
    """The 3 x 3 factor A of the correlated branch (:533-538): cov = |L^2 U^T D U| with L = level2 / 255, D = diag(rand(3)), U =
    orth(rand(3, 3)); n = A z has numpy's `multivariate_normal(0, cov)` law for z ~ N(0, I) (its SVD factor: cov = u s v, A =
    (sqrt(s) v)^T)."""
    from scipy.linalg import orth
    L = level2 / 255.0
    D = np.diag(rng.random(3))
    U = orth(rng.random((3, 3)))
    cov = np.abs(L ** 2 * (U.T @ D @ U))
    _, s, v = np.linalg.svd(cov)
    return (np.sqrt(s)[:, None] * v).T


def _draw_noise(rng, n, c, speckle):
    """`add_Gaussian_noise` / `add_speckle_noise` (:526-558) for n images: level randint(2, 25) / 255; per band with probability
    0.4, one plane for all bands with 0.4, else 3-band correlated (c == 3 only: else per band).  Speckle is on with probability
    0.1 per image (:732, :750)."""
    on = rng.random(n) < 0.1 if speckle else np.ones(n, dtype=bool)
    level = rng.integers(2, 26, n)
    rnum = rng.random(n)
    branch = np.where(rnum > 0.6, BRANCH_BAND, np.where(rnum < 0.4, BRANCH_GRAY, BRANCH_CORR)).astype(np.int32)
    if c != 3:
        branch[branch == BRANCH_CORR] = BRANCH_BAND
    A = np.zeros((n, 3, 3))
    for i in np.flatnonzero(branch == BRANCH_CORR):  # (an SVD and an orth each: only where the branch needs one)
        A[i] = covariance_factor(rng)
    return {"op": "speckle" if speckle else "noise", "on": on, "level": level, "sigma": level / 255.0, "branch": branch, "A": A}


def _draw_poisson(rng, n, c):
    """`add_Poisson_noise` (:561-572), on with probability 0.1 per image: vals = 10^(2 U + 2); per band with probability 1/2, else
    one gray draw for all bands (c == 3 only)."""
    on = rng.random(n) < 0.1
    vals = 10 ** (2 * rng.random(n) + 2.0)
    gray = rng.random(n) >= 0.5
    if c != 3:
        gray[:] = False
    return {"op": "poisson", "on": on, "vals": vals, "gray": gray}


def draw_recipe(rng, n, c, h, w, sf, kind="plus", shuffle_prob=0.5):
    """One batch's recipe: {"kind", "n", "c", "h", "w", "sf", "sharpen", "order", "ops"}.  `order` is the slot order, `ops` the
    ops in the order they run - the slots ("isp" included: a no-op), then the final resize to (h // sf, w // sf) and, for kind
    "plus" with 3 bands, the final JPEG; every op dict has "op" and "slot" (a slot index, or "final") and its parameters: scalars
    for what the batch shares (resize), arrays of n for what is per image."""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r} must be one of {KINDS}")
    if n < 1 or c < 1 or h // sf < 1 or w // sf < 1:
        raise ValueError(f"draw_recipe: n={n} c={c} h={h} w={w} sf={sf}")
    slots = PLUS_SLOTS if kind == "plus" else SOFT_SLOTS
    shuffled = rng.random() < shuffle_prob
    order = np.arange(len(slots))
    if kind == "soft" or shuffled:
        order = rng.permutation(len(slots))
    else:  # the local shuffles of the two noise groups (:716-717)
        order[2:6] = rng.permutation(order[2:6])
        order[9:13] = rng.permutation(order[9:13])
    ops, ch, cw = [], h, w
    for slot in order.tolist():
        name = slots[slot]
        if name == "blur":
            op = _draw_blur(rng, n, sf)
        elif name == "resize":
            op = _draw_resize(rng, sf, ch, cw)
            ch, cw = op["out_h"], op["out_w"]
        elif name == "noise":
            op = _draw_noise(rng, n, c, speckle=False)
        elif name == "speckle":
            op = _draw_noise(rng, n, c, speckle=True)
        elif name == "poisson":
            op = _draw_poisson(rng, n, c)
        elif name == "jpeg":
            op = {"op": "jpeg", "quality": rng.integers(30, 96, n).astype(np.int32)}
            if c != 3:
                op = {"op": "skip"}
        else:
            op = {"op": "isp"}
        op["slot"] = slot
        ops.append(op)
    ops.append({"op": "resize", "slot": "final", "factor": None, "mode": int(rng.integers(1, 4)), "out_h": h // sf, "out_w": w // sf})
    if kind == "plus":
        quality = rng.integers(30, 96, n).astype(np.int32)
        if c == 3:
            ops.append({"op": "jpeg", "slot": "final", "quality": quality})
    return {"kind": kind, "n": n, "c": c, "h": h, "w": w, "sf": sf, "sharpen": kind == "plus", "shuffled": bool(shuffled),
            "order": order.tolist(), "ops": ops}


# ---------------------------------------------------------------------------------------------
# ops (device)
# ---------------------------------------------------------------------------------------------
def _check(what, x, dtype=torch.float32, dim=4):
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != dtype or x.dim() != dim or not x.is_contiguous():
        raise RuntimeError(f"{what}: expected a contiguous {dim}-d {dtype} tensor on a ROCm device (no CPU fallback)")
    return x


def _stream(x):
    return C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _host_taps(taps):
    taps = np.ascontiguousarray(taps, dtype=np.float32)
    return taps, taps.ctypes.data_as(C.POINTER(C.c_float)), int(taps.shape[0])


def blur(x, kernels, ksizes=None):
    """x (N, C, H, W) convolved with kernels[n] (N, K, K fp32 on the device; K odd, <= 25) on the reflect-101 border; `ksizes` (N
    int32 on the device, optional): image n's kernel is the centred ksizes[n]-sized part of its table (drs_bsr_blur)."""
    x, kernels = _check("blur", x), _check("blur: kernels", kernels, dim=3)
    n, c, h, w = x.shape
    if kernels.shape[0] != n or kernels.shape[1] != kernels.shape[2]:
        raise RuntimeError(f"blur: kernels {tuple(kernels.shape)} for a batch of {n}")
    if ksizes is not None and (_check("blur: ksizes", ksizes, torch.int32, 1).shape[0] != n):
        raise RuntimeError(f"blur: {ksizes.shape[0]} kernel sizes for a batch of {n}")
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.load().drs_bsr_blur(_ptr(x), _ptr(out), _ptr(kernels), _ptr(ksizes), n, c, h, w, kernels.shape[1], _stream(x))
    _lib.check(st, "drs_bsr_blur")
    return out


def blur_sep(x, taps):
    """x convolved with taps (*) taps^T, one 1-D kernel of up to 51 taps (host array) for every plane (drs_bsr_blur_sep)."""
    x = _check("blur_sep", x)
    n, c, h, w = x.shape
    keep, tp, k = _host_taps(taps)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.load().drs_bsr_blur_sep(_ptr(x), _ptr(out), tp, k, n, c, h, w, _stream(x))
    _lib.check(st, "drs_bsr_blur_sep")
    return out


def sharpen(x, taps=None, weight=USM_WEIGHT, threshold=USM_THRESHOLD):
    """The reference's `add_sharpening` (:471-495; Real-ESRGAN's USM): see drs_bsr_sharpen.  `taps`: the Gaussian (default: 51
    taps, sigma 8)."""
    x = _check("sharpen", x)
    n, c, h, w = x.shape
    keep, tp, k = _host_taps(usm_taps() if taps is None else taps)
    out, scratch = torch.empty_like(x), torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = _lib.load().drs_bsr_sharpen(_ptr(x), _ptr(out), _ptr(scratch), tp, k, float(weight), float(threshold), n, c, h, w,
                                         _stream(x))
    _lib.check(st, "drs_bsr_sharpen")
    return out


def resize(x, out_h, out_w, mode, quantise=False):
    """x (N, C, H, W) -> (N, C, out_h, out_w) clipped to [0, 1]; mode BILINEAR / BICUBIC / AREA (drs_bsr_resize: the project's
    definitions of cv2's flags 1 / 2 / 3).  `quantise`: returns (out, rint(out * 255) / 255)."""
    x = _check("resize", x)
    n, c, h, w = x.shape
    out = torch.empty((n, c, int(out_h), int(out_w)), dtype=torch.float32, device=x.device)
    out_q = torch.empty_like(out) if quantise else None
    with torch.cuda.device(x.device):
        st = _lib.load().drs_bsr_resize(_ptr(x), _ptr(out), _ptr(out_q), n, c, h, w, int(out_h), int(out_w), int(mode), _stream(x))
    _lib.check(st, "drs_bsr_resize")
    return (out, out_q) if quantise else out


def noise_(x, z, mode, par, aux=None):
    """In place on x (N, C, H, W): the per-image noise op of drs_bsr_noise from the draws z (x's shape); mode (N, 2) int32 =
    (kind, branch), par (N, 10) fp32 = (sigma, A row by row), aux (N, H, W) fp32 for the gray Poisson kind - all on the device."""
    x, z = _check("noise_", x), _check("noise_: z", z)
    n, c, h, w = x.shape
    if z.shape != x.shape or tuple(_check("noise_: mode", mode, torch.int32, 2).shape) != (n, 2) or \
            tuple(_check("noise_: par", par, dim=2).shape) != (n, 10):
        raise RuntimeError(f"noise_: z {tuple(z.shape)}, mode {tuple(mode.shape)}, par {tuple(par.shape)} for x {tuple(x.shape)}")
    if aux is not None and tuple(_check("noise_: aux", aux, dim=3).shape) != (n, h, w):
        raise RuntimeError(f"noise_: aux {tuple(aux.shape)} for x {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        st = _lib.load().drs_bsr_noise(_ptr(x), _ptr(z), _ptr(aux), _ptr(mode), _ptr(par), n, c, h, w, _stream(x))
    _lib.check(st, "drs_bsr_noise")
    return x


def jpeg(x, quality):
    """The JPEG round trip of x (N, 3, H, W) at quality[n] (N int32 on the device): drs_bsr_jpeg.  The result lies on k / 255."""
    x = _check("jpeg", x)
    n, c, h, w = x.shape
    if c != 3 or _check("jpeg: quality", quality, torch.int32, 1).shape[0] != n:
        raise RuntimeError(f"jpeg: x {tuple(x.shape)} needs 3 bands and {n} qualities")
    lib = _lib.load()
    nbytes = lib.drs_bsr_jpeg_scratch_bytes(n, h, w)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        st = lib.drs_bsr_jpeg(_ptr(x), _ptr(out), _ptr(quality), n, h, w, _ptr(scratch), nbytes, _stream(x))
    _lib.check(st, "drs_bsr_jpeg")
    return out


def noise_params(op):
    """(mode (n, 2) int32, par (n, 10) float32) host arrays of a recipe's noise / speckle / poisson op (drs_bsr_noise)."""
    n = len(op["on"])
    mode, par = np.zeros((n, 2), dtype=np.int32), np.zeros((n, 10), dtype=np.float32)
    if op["op"] == "poisson":
        mode[:, 0] = np.where(op["on"], np.where(op["gray"], NOISE_POISSON_GRAY, NOISE_POISSON), NOISE_OFF)
        par[:, 0] = op["vals"]
    else:
        mode[:, 0] = np.where(op["on"], NOISE_SPECKLE if op["op"] == "speckle" else NOISE_ADD, NOISE_OFF)
        mode[:, 1] = op["branch"]
        par[:, 0] = op["sigma"]
        par[:, 1:] = op["A"].reshape(n, 9)
    return mode, par


def poisson_rate(x, mode, par):
    """The Poisson rates of drs_bsr_noise's kinds 3 / 4 for x (N, C, H, W): q(x) vals per band, and for a gray image (kind 4) in
    band 0 gray(q(x)) vals with the gray LEVEL formed in integers, (299 R + 587 G + 114 B + 500) // 1000.  fp32, on the device."""
    n, c = x.shape[:2]
    q = (x.clamp(0, 1) * 255).round()
    vals = par[:, 0].view(n, 1, 1, 1)
    rate = q / 255 * vals
    if c == 3:
        lv = q.to(torch.int64)
        g = ((299 * lv[:, 0] + 587 * lv[:, 1] + 114 * lv[:, 2] + 500) // 1000).to(torch.float32)
        is_gray = (mode[:, 0] == NOISE_POISSON_GRAY).view(n, 1, 1)
        rate[:, 0] = torch.where(is_gray, g / 255 * vals.view(n, 1, 1), rate[:, 0])
    return rate


def _upload(recipe, device):
    """Every per-image parameter of the recipe on the device, in one float and one int upload: {op index: tensors}."""
    fl, it, where = [], [], {}

    def put(lst, a):
        pos = sum(b.size for b in lst)
        lst.append(np.ascontiguousarray(a).reshape(-1))
        return pos
    for i, op in enumerate(recipe["ops"]):
        if op["op"] == "blur":
            where[i] = ("blur", put(fl, op["kernels"]), op["kernels"].shape, put(it, op["ksize"]))
        elif op["op"] in ("noise", "speckle", "poisson"):
            mode, par = noise_params(op)
            where[i] = ("noise", put(fl, par), put(it, mode))
        elif op["op"] == "jpeg":
            where[i] = ("jpeg", put(it, op["quality"]))
    n = recipe["n"]
    pin = torch.cuda.is_available()
    fbuf = torch.from_numpy(np.concatenate(fl).astype(np.float32) if fl else np.zeros(1, np.float32))
    ibuf = torch.from_numpy(np.concatenate(it).astype(np.int32) if it else np.zeros(1, np.int32))
    if pin:
        fbuf, ibuf = fbuf.pin_memory(), ibuf.pin_memory()
    fd, idv = fbuf.to(device, non_blocking=True), ibuf.to(device, non_blocking=True)
    out = {}
    for i, w in where.items():
        if w[0] == "blur":
            _, f, shape, j = w
            out[i] = (fd[f:f + int(np.prod(shape))].view(shape), idv[j:j + n])
        elif w[0] == "noise":
            out[i] = (idv[w[2]:w[2] + 2 * n].view(n, 2), fd[w[1]:w[1] + 10 * n].view(n, 10))
        else:
            out[i] = (idv[w[1]:w[1] + n],)
    return out


def degrade(hr, recipe, return_intermediates=False, generator=None):
    """(lr, hr_out) for hr (N, C, H, W) float32 in [0, 1] on a ROCm device under `recipe` (draw_recipe): hr_out is the USM of hr
    for a sharpening recipe (else hr itself), lr (N, C, H // sf, W // sf) lies in [0, 1] on the k / 255 grid.  The normal and
    Poisson draws come from `generator` (a torch.Generator of hr's device; None: the device's default).
    `return_intermediates`: also the list of stages, one dict per launch that changed the batch - {"op", "slot", "inp" (the
    batch before), "out" (after), the recipe's op under "params", and "z" / "aux" / "rate" / "mode" / "par" for the noise ops}."""
    hr = _check("degrade", hr)
    n, c, h, w = hr.shape
    if (n, c, h, w) != (recipe["n"], recipe["c"], recipe["h"], recipe["w"]):
        raise RuntimeError(f"degrade: a batch {tuple(hr.shape)} under a recipe for {(recipe['n'], recipe['c'], recipe['h'], recipe['w'])}")
    dev = _upload(recipe, hr.device)
    stages = []

    def note(op, inp, out, **more):
        if return_intermediates:
            stages.append({"op": op["op"], "slot": op.get("slot"), "params": op, "inp": inp.clone(), "out": out.clone(), **more})
    if recipe["sharpen"]:
        hr_out = sharpen(hr)
        note({"op": "sharpen", "slot": "first"}, hr, hr_out)
    else:
        hr_out = hr
    x = hr_out
    last = len(recipe["ops"]) - 1
    for i, op in enumerate(recipe["ops"]):
        name = op["op"]
        if name == "blur":
            y = blur(x, *dev[i])
            note(op, x, y)
            x = y
        elif name == "resize":
            if op["slot"] == "final":
                y, yq = resize(x, op["out_h"], op["out_w"], op["mode"], quantise=True)
                note(op, x, y)
                if i == last:  # no JPEG follows: the LR image is the quantised copy (JPEG quantises its input itself)
                    note({"op": "quantise", "slot": "final"}, y, yq)
                    y = yq
            else:
                y = resize(x, op["out_h"], op["out_w"], op["mode"])
                note(op, x, y)
            x = y
        elif name in ("noise", "speckle", "poisson"):
            if not op["on"].any():
                continue
            mode, par = dev[i]
            if x is hr_out:
                x = x.clone()  # (the noise op works in place: the HR output keeps its values)
            before = x.clone() if return_intermediates else None
            rate = None
            if name == "poisson":
                rate = poisson_rate(x, mode, par)
                z = torch.poisson(rate, generator=generator)
                aux = rate[:, 0].contiguous()
            else:
                z = torch.randn(x.shape, dtype=torch.float32, device=x.device, generator=generator)
                aux = None
            noise_(x, z, mode, par, aux)
            if return_intermediates:
                note(op, before, x, z=z, aux=aux, rate=rate, mode=mode.clone(), par=par.clone())
        elif name == "jpeg":
            y = jpeg(x, *dev[i])
            note(op, x, y, quality=dev[i][0].clone())
            x = y
    return (x, hr_out, stages) if return_intermediates else (x, hr_out)


# ---------------------------------------------------------------------------------------------
# feed
# ---------------------------------------------------------------------------------------------
class DeviceBSRFeed:
    """Iterable of (lr, hr) float32 batches in [0, 1] like `DeviceSuperresFeed`, under the blind degradation: `hr_u8` (L, C, S, S)
    uint8 on the device, LR S // m on a side.  Every batch draws a fresh recipe (`draw_recipe`, kind "plus" or "soft") and fresh
    noise from generators seeded with `seed`: two feeds with one seed yield the same batches; the epochs of one feed differ,
    unless it is `fixed` - then every `__iter__` starts from the seed again (the validation feed: the reference's frozen
    validation set, so validation losses compare across epochs).

    `crop_size` / `augment` ("none", "flip", "d4") make the feed active (augment.py): every item is a
    crop_size window of its cache image (default: the whole, square image) under a symmetry of the mode, drawn from the feed's own
    `np.random.default_rng([augment_seed, augment_rank])` - not from the recipe or noise generators; the recipe is drawn for the
    window's size; an epoch is `num_crops` passes over the cache; `fixed_crop`: the centre window, no symmetry, one pass.
    `last_items`: the last batch's (n, 4) host items (src, y0, x0, code)."""

    def __init__(self, hr_u8, magnification_factor, batch_size=16, shuffle=True, kind="plus", seed=0, fixed=False, crop_size=None,
                 augment="none", num_crops=1, augment_seed=0, augment_rank=0, fixed_crop=False):
        if kind not in KINDS:
            raise ValueError(f"kind={kind!r} must be one of {KINDS}")
        if not isinstance(hr_u8, torch.Tensor) or not hr_u8.is_cuda or hr_u8.dtype != torch.uint8 or hr_u8.dim() != 4:
            raise RuntimeError("DeviceBSRFeed: hr must be a (L, C, H, W) uint8 tensor on a ROCm device (no CPU fallback)")
        m = int(magnification_factor)
        if m < 1 or hr_u8.shape[2] // m < 1 or hr_u8.shape[3] // m < 1:
            raise RuntimeError(f"DeviceBSRFeed: {hr_u8.shape[2]}x{hr_u8.shape[3]} is too small for magnification {m}")
        self.hr = hr_u8.contiguous()
        self.magnification_factor = m
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.kind = kind
        self.seed = int(seed)
        self.fixed = fixed
        self._labels = torch.zeros(self.hr.shape[0], dtype=torch.int64, device=self.hr.device)
        self._aug = None
        if crop_size is not None or augment != "none":
            from .augment import FeedAugment
            self._aug = FeedAugment(self.hr.shape[2], self.hr.shape[3], crop_size, augment, num_crops, augment_seed, augment_rank,
                                    fixed_crop)
            if self._aug.size // m < 1:
                raise RuntimeError(f"DeviceBSRFeed: windows of {self._aug.size} are too small for magnification {m}")
        self.last_items = None
        self._seed_generators()

    def _seed_generators(self):
        self._rng = np.random.default_rng(self.seed)
        self._gen = torch.Generator(device=self.hr.device).manual_seed(self.seed)

    def __len__(self):
        if self._aug is not None:
            return self._aug.num_batches(self.hr.shape[0], self.batch_size)
        return (self.hr.shape[0] + self.batch_size - 1) // self.batch_size

    def _batch(self, idx, rng, gen):
        from .feeds import gather_u8
        hr = gather_u8(self.hr, self._labels, idx)[0]
        n, c, h, w = hr.shape
        return degrade(hr, draw_recipe(rng, n, c, h, w, self.magnification_factor, self.kind), generator=gen)

    def _batch_items(self, items, rng, gen):
        """`_batch` of an active feed: the windows of `items` as float(b) / 255 (what `gather_u8` makes of whole images), degraded
        under a recipe for the window's size."""
        from .augment import crop_d4_u8_f32, upload_items
        hr = crop_d4_u8_f32(self.hr, self._labels, upload_items(items, self.hr.device), self._aug.size)[0]
        n, c, h, w = hr.shape
        return degrade(hr, draw_recipe(rng, n, c, h, w, self.magnification_factor, self.kind), generator=gen)

    def item(self, idx):
        """(x, y) of dataset item `idx`, (C, h, w) / (C, H, W), under a recipe and noise that depend on (seed, idx) alone: the
        same on every call, and no draw of the feed's own streams is consumed."""
        idx = int(idx)
        rng = np.random.default_rng([self.seed, idx])
        gen = torch.Generator(device=self.hr.device).manual_seed(self.seed * 1000003 + idx)
        if self._aug is not None:  # the centre window, no symmetry
            if not 0 <= idx < self.hr.shape[0]:
                raise IndexError(f"item {idx} of a dataset of {self.hr.shape[0]}")
            x, y = self._batch_items(self._aug.centre(idx), rng, gen)
            return x[0], y[0]
        x, y = self._batch(torch.tensor([idx], dtype=torch.int64, device=self.hr.device), rng, gen)
        return x[0], y[0]

    def epoch_order(self):
        """The index vector of one epoch of an active feed, on the host: `num_crops` orders drawn as one is drawn today."""
        n = self.hr.shape[0]
        return self._aug.epoch_order(lambda: torch.from_numpy(self._rng.permutation(n) if self.shuffle else np.arange(n)))

    def __iter__(self):
        if self.fixed:
            self._seed_generators()
        if self._aug is not None:
            order = self.epoch_order().numpy()
            for i in range(0, order.shape[0], self.batch_size):
                self.last_items = self._aug.items(order[i:i + self.batch_size])
                yield self._batch_items(self.last_items, self._rng, self._gen)
            return
        n = self.hr.shape[0]
        order = torch.from_numpy(self._rng.permutation(n) if self.shuffle else np.arange(n)).to(self.hr.device)
        for i in range(0, n, self.batch_size):
            yield self._batch(order[i:i + self.batch_size], self._rng, self._gen)
