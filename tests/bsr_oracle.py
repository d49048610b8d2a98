"""Float64 / integer oracle of the blind-degradation ops (include/drs_hip.h: drs_bsr_*), numpy + scipy only.
Restated from the definitions, not from the kernels: borders through index arrays, resizes as weight matrices built from exact
rationals, the JPEG round trip in int64."""
import numpy as np

EPS = 2.0 ** -24


def _np(x, dtype=np.float64):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=dtype)


def reflect101(i, n):
    """Index i of an axis of n samples continued by reflection about the edge samples' centres, as often as needed."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


# ---- blur -------------------------------------------------------------------------------------------------------------------
def blur_plane(img, k):
    """True convolution of a 2-d float64 image with an odd-sized kernel on the reflect-101 border."""
    img, k = np.asarray(img, dtype=np.float64), np.asarray(k, dtype=np.float64)
    H, W = img.shape
    ry, rx = k.shape[0] // 2, k.shape[1] // 2
    pad = img[reflect101(np.arange(-ry, H + ry), H)][:, reflect101(np.arange(-rx, W + rx), W)]
    out = np.zeros((H, W))
    for i in range(k.shape[0]):
        for j in range(k.shape[1]):
            if k[i, j] != 0.0:
                out += k[i, j] * pad[2 * ry - i:2 * ry - i + H, 2 * rx - j:2 * rx - j + W]  # in(y + r - i, x + r - j)
    return out


def blur(x, kernels, ksizes=None):
    """drs_bsr_blur: image n under the centred ksizes[n]-sized part of kernels[n] (N, K, K)."""
    x, kernels = _np(x), _np(kernels)
    out = np.empty_like(x)
    K = kernels.shape[1]
    for n in range(x.shape[0]):
        ks = K if ksizes is None else int(ksizes[n])
        o = (K - ks) // 2
        for c in range(x.shape[1]):
            out[n, c] = blur_plane(x[n, c], kernels[n, o:o + ks, o:o + ks])
    return out


def blur_sep(x, taps):
    x, taps = _np(x), _np(taps)
    out = np.empty_like(x)
    for n in range(x.shape[0]):
        for c in range(x.shape[1]):
            out[n, c] = blur_plane(blur_plane(x[n, c], taps[None, :]), taps[:, None])
    return out


def gaussian_taps(k=51):
    """cv2.GaussianBlur(img, (k, k), 0): sigma = 0.3 ((k - 1) / 2 - 1) + 0.8."""
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    t = np.arange(k) - (k - 1) / 2
    g = np.exp(-t * t / (2 * sigma * sigma))
    return g / g.sum()


def usm(x, taps, weight=0.5, threshold=10.0, ambiguous=0.0):
    """drs_bsr_sharpen in float64 as (low, high): the mask |x - blur| * 255 > threshold is a step, so a pixel within `ambiguous` of
    the step is taken both ways - the result is monotone in the mask pixel by pixel (soft = blur(mask) with non-negative taps,
    out = x + soft (sharp - x)), so the true result for any resolution of those pixels lies between the two."""
    x = _np(x)
    b = blur_sep(x, taps)
    d = np.abs(x - b) * 255 - threshold
    sharp = np.clip(x + weight * (x - b), 0, 1)
    outs = []
    for m in (d > ambiguous, d > -ambiguous):
        soft = blur_sep(m.astype(np.float64), taps)
        outs.append(soft * sharp + (1 - soft) * x)
    return np.minimum(*outs), np.maximum(*outs)


# ---- resize -----------------------------------------------------------------------------------------------------------------
def cubic_weights(f, a=-0.75):
    """The cubic convolution kernel at distances 1 + f, f, 1 - f, 2 - f."""
    def near(t):
        return ((a + 2) * t - (a + 3)) * t * t + 1

    def far(t):
        return ((a * t - 5 * a) * t + 8 * a) * t - 4 * a
    return np.array([far(1 + f), near(f), near(1 - f), far(2 - f)])


def axis_matrix(n_in, n_out, mode):
    """(n_out, n_in) weights of one axis: mode 1 bilinear, 2 bicubic, 3 area (the box mean where the axis shrinks, else
    bilinear); half-pixel centres, border replicated.  Positions are exact rationals: (2 o + 1) n_in - n_out over 2 n_out."""
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        if mode == 3 and n_in > n_out:
            for s in range(n_in):
                ov = min((o + 1) * n_in, (s + 1) * n_out) - max(o * n_in, s * n_out)
                if ov > 0:
                    M[o, s] += ov / n_in
            continue
        num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
        q = num // den
        f = (num - q * den) / den
        taps = zip(range(q - 1, q + 3), cubic_weights(f)) if mode == 2 else ((q, 1 - f), (q + 1, f))
        for s, wgt in taps:
            M[o, min(max(s, 0), n_in - 1)] += wgt
    return M


def resize(x, out_h, out_w, mode):
    x = _np(x)
    My, Mx = axis_matrix(x.shape[2], out_h, mode), axis_matrix(x.shape[3], out_w, mode)
    return np.clip(np.einsum("oh,nchw,pw->ncop", My, x, Mx), 0, 1)


def resize_abs_weight(n_in, n_out, mode):
    """max over outputs of sum |w| of the axis (1 for the non-negative modes)."""
    return np.abs(axis_matrix(n_in, n_out, mode)).sum(axis=1).max()


def quantise(x32):
    """rint(x * 255) / 255 in float32, as the kernels do it."""
    x32 = _np(x32, np.float32)
    return (np.rint(np.clip(x32, np.float32(0), np.float32(1)) * np.float32(255)) / np.float32(255)).astype(np.float32)


# ---- noise ------------------------------------------------------------------------------------------------------------------
def noise(x, z, mode, par, aux=None):
    """drs_bsr_noise in float64 (q(x) in float32 arithmetic, as defined)."""
    x32 = _np(x, np.float32)
    x, z, mode, par = _np(x), _np(z), _np(mode, np.int64), _np(par)
    out = x.copy()
    N, C = x.shape[:2]
    for n in range(N):
        kind, branch = mode[n]
        sigma, A = par[n, 0], par[n, 1:].reshape(3, 3)
        if branch == 2 and C != 3:
            branch = 0
        if kind == 3:
            out[n] = np.clip(z[n] / sigma, 0, 1)
        elif kind == 4:
            if aux is None:
                continue
            out[n] = np.clip(quantise(x32[n]).astype(np.float64) + (z[n, 0] - _np(aux)[n]) / sigma, 0, 1)
        elif kind in (1, 2):
            if branch == 0:
                nv = sigma * z[n]
            elif branch == 1:
                nv = np.broadcast_to(sigma * z[n, 0], x[n].shape)
            else:
                nv = np.einsum("ij,jhw->ihw", A, z[n])
            v = x[n] if kind == 1 else np.clip(x[n], 0, 1)
            out[n] = np.clip(v + nv, 0, 1) if kind == 1 else np.clip(v + v * nv, 0, 1)
    return out


def poisson_rate(x, mode, par):
    """bsr.poisson_rate in float32 arithmetic: q(x) vals per band; band 0 of a gray image gray(q(x)) vals with the integer gray level."""
    x32, mode = _np(x, np.float32), _np(mode, np.int64)
    vals = _np(par, np.float32)[:, 0].reshape(-1, 1, 1, 1)
    q = np.rint(np.clip(x32, np.float32(0), np.float32(1)) * np.float32(255))
    rate = q / np.float32(255) * vals
    if x32.shape[1] == 3:
        lv = q.astype(np.int64)
        g = ((299 * lv[:, 0] + 587 * lv[:, 1] + 114 * lv[:, 2] + 500) // 1000).astype(np.float32)
        gray = (mode[:, 0] == 4).reshape(-1, 1, 1)
        rate[:, 0] = np.where(gray, g / np.float32(255) * vals[:, 0], rate[:, 0])
    return rate.astype(np.float32)


# ---- JPEG ------------------------------------------------------------------------------------------------------------------
DCT = np.array([[5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793],
                [8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035],
                [7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568],
                [6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811],
                [5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793],
                [4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551],
                [3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135],
                [1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598]], dtype=np.int64)
# ITU-T T.81 Annex K, tables K.1 and K.2
QUANT = np.array([[16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                  [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32], dtype=np.int64).reshape(2, 8, 8)


def dct_matrix():
    """C[u][x] = round(2^14 (c_u / 2) cos((2 x + 1) u pi / 16)), c_0 = 1 / sqrt 2: what DCT spells out."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, 1 / np.sqrt(2), 1.0)
    return np.round(2 ** 14 * 0.5 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


def quant_table(which, quality):
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((QUANT[which] * scale + 50) // 100, 1, 255)


def _blocks(plane):
    """(H, W) -> (H / 8, W / 8, 8, 8)."""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    return b.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8)


def _codec(plane, Q):
    """8 x 8 blocks of an int64 plane of samples 0 .. 255 through DCT, quantisation, dequantisation and inverse DCT."""
    s = _blocks(plane) - 128                                         # [.., y, x]
    t = (np.einsum("vx,abyx->abyv", DCT, s) + 256) >> 9
    F = np.einsum("uy,abyv->abuv", DCT, t)
    mag = (np.abs(F) + (Q << 18)) // (Q << 19)
    D = np.sign(F) * mag * Q
    t = (np.einsum("uy,abuv->abyv", DCT, D) + 256) >> 9
    p = np.einsum("vx,abyv->abyx", DCT, t)
    return _unblocks(np.clip(((p + (1 << 18)) >> 19) + 128, 0, 255))


def jpeg_u8(rgb, quality):
    """The round trip of one (H, W, 3) uint8 image: (H, W, 3) uint8."""
    rgb = np.asarray(rgb).astype(np.int64)
    H, W = rgb.shape[:2]
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    rgb = rgb[np.minimum(np.arange(Hp), H - 1)][:, np.minimum(np.arange(Wp), W - 1)]
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    bias = 1 + (np.arange(Wp // 2) & 1)[None, :]

    def down(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
    Y = _codec(Y, quant_table(0, quality))
    Cb, Cr = _codec(down(Cb), quant_table(1, quality)), _codec(down(Cr), quant_table(1, quality))
    Hc, Wc = Hp // 2, Wp // 2
    y, x = np.arange(Hp), np.arange(Wp)
    cy, cx = y >> 1, x >> 1
    yn = np.where(y & 1, np.minimum(cy + 1, Hc - 1), np.maximum(cy - 1, 0))
    xn = np.where(x & 1, np.minimum(cx + 1, Wc - 1), np.maximum(cx - 1, 0))
    xbias = np.where(x & 1, 7, 8)[None, :]

    def up(c):
        col = 3 * c[cy] + c[yn]                                     # (Hp, Wc)
        return (3 * col[:, cx] + col[:, xn] + xbias) >> 4
    cb, cr = up(Cb) - 128, up(Cr) - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16), Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255)[:H, :W].astype(np.uint8)


def jpeg(x, quality):
    """drs_bsr_jpeg: (N, 3, H, W) float32 -> float32, bit for bit."""
    x32 = _np(x, np.float32)
    lv = np.rint(np.clip(x32, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    out = np.stack([jpeg_u8(lv[n].transpose(1, 2, 0), int(quality[n])).transpose(2, 0, 1) for n in range(x32.shape[0])])
    return out.astype(np.float32) / np.float32(255)
