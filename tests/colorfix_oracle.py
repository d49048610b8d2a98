"""Float64 restatement of the two colour corrections of diffusionremotesensing_amd/colorfix.py, from the published formulas
(the wavelet reconstruction and the AdaIN colour fix StableSR ships): the oracle of tests/test_colorfix_host.py and
tests/test_gpu_colorfix.py."""
import torch
import torch.nn.functional as F

KERNEL = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)


def blur(x, d):
    """The 3 x 3 binomial kernel of dilation d on replicate padding of width d, per plane of (B, C, H, W) float64."""
    B, C, H, W = x.shape
    k = torch.outer(KERNEL, KERNEL).expand(C, 1, 3, 3).contiguous()
    # (F.pad's replicate mode takes any width, also one beyond the image)
    return F.conv2d(F.pad(x, (d, d, d, d), mode="replicate"), k, dilation=d, groups=C)


def blur_by_index(plane, d):
    """The definition, element by element, on one (H, W) plane: sum k_i k_j x[clamp(y + i d)][clamp(x + j d)]."""
    H, W = plane.shape
    out = torch.zeros_like(plane)
    for y in range(H):
        for x in range(W):
            for i in (-1, 0, 1):
                for j in (-1, 0, 1):
                    out[y, x] += KERNEL[i + 1] * KERNEL[j + 1] * plane[min(max(y + i * d, 0), H - 1), min(max(x + j * d, 0), W - 1)]
    return out


def decompose(x, levels):
    """(high, low) of the wavelet decomposition: low = blur_{2^(L-1)} o ... o blur_1 (x), high = the sum of the differences."""
    high, low = torch.zeros_like(x), x
    for i in range(levels):
        nxt = blur(low, 2 ** i)
        high += low - nxt
        low = nxt
    return high, low


def wavelet(sr, guide, levels=5):
    """The high frequencies of sr on the low frequencies of guide, float64."""
    high, _ = decompose(sr.double(), levels)
    _, low = decompose(guide.double(), levels)
    return high + low


def adain_coefficients(sr, guide):
    """(a, b) per plane, (B, C, 1, 1) float64: out = a sr + b."""
    sr, guide = sr.double(), guide.double()
    mean_s, mean_g = sr.mean(dim=(2, 3), keepdim=True), guide.mean(dim=(2, 3), keepdim=True)
    std_s = torch.sqrt(sr.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    std_g = torch.sqrt(guide.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    a = std_g / std_s
    return a, mean_g - a * mean_s


def adain(sr, guide):
    sr, guide = sr.double(), guide.double()
    mean_s, mean_g = sr.mean(dim=(2, 3), keepdim=True), guide.mean(dim=(2, 3), keepdim=True)
    std_s = torch.sqrt(sr.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    std_g = torch.sqrt(guide.var(dim=(2, 3), unbiased=True, keepdim=True) + 1e-5)
    return (sr - mean_s) / std_s * std_g + mean_g
