"""Thin torch-tensor wrappers over the operator-level C-ABI entries (include/drs_hip.h).

PyTorch is used only for device memory and the current stream.  Every wrapper requires
ROCm-device fp32 contiguous tensors and raises otherwise: there is no CPU path.
"""
import ctypes as C
import math

import torch

from . import _lib


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _req(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the HIP path needs a ROCm device tensor (no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _req_state(x, op, name="x"):  # the tensor an in-place step updates is used as it is
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.dtype == torch.float32):
        raise RuntimeError(f"{op}: {name} must be a contiguous fp32 ROCm tensor (no CPU fallback)")


def _req_numel(op, x, named, state="x"):  # named = ((name, tensor or None), ...): as many elements as the state x
    for name, t in named:
        if t is not None and t.numel() != x.numel():
            raise RuntimeError(f"{op}: {name} has {t.numel()} elements, {state} has {x.numel()}")


def conv2d(x, w, b=None, stride=1, padding=0, transposed=False, output_padding=0, relu=False, impl="direct"):
    """F.conv2d / F.conv_transpose2d for the flavours the UNet uses (NCHW, fp32)."""
    lib = _lib.load()
    x = _req(x, "x"); w = _req(w, "w")
    if b is not None:
        b = _req(b, "b")
    N, Cin, H, W = x.shape
    if transposed:
        if w.shape[0] != Cin:
            raise RuntimeError(f"conv_transpose2d: weight {tuple(w.shape)} does not match Cin={Cin}")
        Cout = w.shape[1]
    else:
        if w.shape[1] != Cin:
            raise RuntimeError(f"conv2d: weight {tuple(w.shape)} does not match Cin={Cin}")
        Cout = w.shape[0]
    KH, KW = w.shape[2], w.shape[3]
    if transposed:
        OH = (H - 1) * stride - 2 * padding + KH + output_padding
        OW = (W - 1) * stride - 2 * padding + KW + output_padding
    else:
        OH = (H + 2 * padding - KH) // stride + 1
        OW = (W + 2 * padding - KW) // stride + 1
    y = torch.empty((N, Cout, max(OH, 0), max(OW, 0)), dtype=torch.float32, device=x.device)
    args = (N, Cin, H, W, Cout, KH, KW, stride, padding, int(transposed), output_padding)
    nbytes = lib.drs_conv2d_workspace_bytes(*args)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    impl_id = _lib.IMPL_BY_NAME[impl] if isinstance(impl, str) else int(impl)
    with torch.cuda.device(x.device):
        st = lib.drs_conv2d_nchw(_ptr(x), _ptr(w), _ptr(b), _ptr(y), *args, int(relu), _ptr(ws), nbytes, impl_id,
                                 _stream(x.device))
    _lib.check(st, "drs_conv2d_nchw")
    return y


def upconv_fused(h, att, t_w, t_b, v_w, v_b, post2=None, fuse_w=None, fuse_b=None):
    """conv2d(cat([conv_transpose2d(h, t_w, t_b, 2, 1, 1), att], 1), v_w, v_b, padding=1) the way the eval plan runs a
    decoder stage: transposed convolution and the x-half of the 3x3 convolution composed into one stride-2 transposed
    convolution (include/drs_hip.h: drs_upconv_fused_nchw).  Returns y, or (y, y + post2[:, :, None, None]) with
    `post2` (N, Ch), or conv1x1(y, fuse_w, fuse_b) with `fuse_w` (fuse_dim, Ch)."""
    lib = _lib.load()
    h = _req(h, "h"); att = _req(att, "att"); t_w = _req(t_w, "t_w"); t_b = _req(t_b, "t_b")
    v_w = _req(v_w, "v_w"); v_b = _req(v_b, "v_b")
    N, Cc, LH, LW = h.shape
    Ch = v_w.shape[0]
    if att.shape != (N, Ch, 2 * LH, 2 * LW) or v_w.shape[1] != Cc + Ch or tuple(t_w.shape) != (Cc, Cc, 3, 3):
        raise RuntimeError(f"upconv_fused: shapes h {tuple(h.shape)} att {tuple(att.shape)} t_w {tuple(t_w.shape)} "
                           f"v_w {tuple(v_w.shape)} do not fit one decoder stage")
    fd = 0
    if fuse_w is not None:
        fuse_w = _req(fuse_w.reshape(fuse_w.shape[0], -1), "fuse_w"); fuse_b = _req(fuse_b, "fuse_b")
        fd = fuse_w.shape[0]
    if post2 is not None:
        post2 = _req(post2, "post2")
    y = torch.empty((N, fd if fd else Ch, 2 * LH, 2 * LW), dtype=torch.float32, device=h.device)
    y2 = torch.empty_like(y) if post2 is not None else None
    nbytes = lib.drs_upconv_fused_workspace_bytes(N, Cc, Ch, LH, LW)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    with torch.cuda.device(h.device):
        st = lib.drs_upconv_fused_nchw(_ptr(h), _ptr(att), _ptr(t_w), _ptr(t_b), _ptr(v_w), _ptr(v_b), _ptr(post2),
                                       _ptr(fuse_w), _ptr(fuse_b), fd, _ptr(y), _ptr(y2), N, Cc, Ch, LH, LW, _ptr(ws),
                                       nbytes, _stream(h.device))
    _lib.check(st, "drs_upconv_fused_nchw")
    return (y, y2) if y2 is not None else y


def bicubic_upsample(x, scale):
    lib = _lib.load()
    x = _req(x, "x")
    N, Cc, H, W = x.shape
    y = torch.empty((N, Cc, H * scale, W * scale), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.drs_bicubic_upsample_nchw(_ptr(x), _ptr(y), N, Cc, H, W, int(scale), _stream(x.device))
    _lib.check(st, "drs_bicubic_upsample_nchw")
    return y


def inv_freq_table(channels=100):
    """Same expression as reference pos_encoding (UNet_model_superres.py:329-331), on the host."""
    return (1.0 / (10000 ** (torch.arange(0, channels, 2).float() / channels))).contiguous()


_INV_FREQ = {}  # (channels, device) -> the table on the device


def _inv_freq_on(channels, device):
    """`inv_freq_table(channels)` on `device`, uploaded once: an upload from pageable memory per call would make the host wait
    for everything enqueued on the caller's stream."""
    key = (int(channels), device.type, device.index if device.index is not None else torch.cuda.current_device())
    table = _INV_FREQ.get(key)
    if table is None:
        table = _INV_FREQ[key] = inv_freq_table(channels).to(device)
    return table


def time_mlp(t, W1, b1, W2, b2):
    lib = _lib.load()
    t = _req(t, "t", torch.int64)
    W1, b1, W2, b2 = (_req(a, n) for a, n in ((W1, "W1"), (b1, "b1"), (W2, "W2"), (b2, "b2")))
    dim_out, dim_in = W1.shape
    inv = _inv_freq_on(dim_in, t.device)
    out = torch.empty((t.shape[0], dim_out), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        st = lib.drs_time_mlp(_ptr(t), _ptr(inv), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2), _ptr(out), t.shape[0], dim_in,
                              dim_out, _stream(t.device))
    _lib.check(st, "drs_time_mlp")
    return out


def noise_images(x0, eps, t, alpha_hat):
    lib = _lib.load()
    x0 = _req(x0, "x0"); eps = _req(eps, "eps"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    if eps.shape != x0.shape or t.shape[0] != x0.shape[0]:
        raise RuntimeError("noise_images: shape mismatch")
    out = torch.empty_like(x0)
    n = x0.shape[0]
    chw = x0.numel() // n if n else 0
    with torch.cuda.device(x0.device):
        st = lib.drs_noise_images(_ptr(x0), _ptr(eps), _ptr(t), _ptr(alpha_hat), alpha_hat.numel(), _ptr(out), n, chw,
                                  _stream(x0.device))
    _lib.check(st, "drs_noise_images")
    return out


PREDICTIONS = {"eps": 0, "v": 1, "x0": 2}  # include/drs_hip.h: DRS_PRED_*


def noise_v_target(x0, eps, t, alpha_hat):
    """(x_t, v) of a training batch from one launch (include/drs_hip.h: drs_noise_v_target): `noise_images`' x_t and the
    v-prediction target sqrt(alpha_hat[t]) eps - sqrt(1 - alpha_hat[t]) x0.  A t outside the table gives that image NaN."""
    lib = _lib.load()
    x0 = _req(x0, "x0"); eps = _req(eps, "eps"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    _req_numel("noise_v_target", x0, (("eps", eps),), "x0")
    n = x0.shape[0] if x0.dim() else 0
    if t.numel() != n:
        raise RuntimeError(f"noise_v_target: t has {t.numel()} elements, x0 has {n} images")
    x_t, v = torch.empty_like(x0), torch.empty_like(x0)
    chw = x0.numel() // n if n else 0
    with torch.cuda.device(x0.device):
        st = lib.drs_noise_v_target(_ptr(x0), _ptr(eps), _ptr(t), _ptr(alpha_hat), alpha_hat.numel(), _ptr(x_t), _ptr(v), n,
                                    chw, _stream(x0.device))
    _lib.check(st, "drs_noise_v_target")
    return x_t, v


def nodata_rule(nodata):
    """The `nodata_value` of the C-ABI for the package's `nodata` setting: True or "nan" is the NaN rule alone (a NaN), a
    number is that value rounded to fp32 (its bands are compared as fp32) on top of the NaN rule."""
    if nodata is True or (isinstance(nodata, str) and nodata.lower() == "nan"):
        return math.nan
    if nodata is None or nodata is False or isinstance(nodata, str):
        raise ValueError(f"nodata={nodata!r} must be True, 'nan' or a number")
    value = float(nodata)
    if math.isinf(value):
        raise ValueError("nodata must be finite (or NaN / True for the NaN rule alone)")
    return value


def noise_target_nodata(x0, eps, t, alpha_hat, prediction, nodata_value=None, fill=0.5):
    """(x_t, target, valid) of a training batch x0 (n, C, H, W) whose no-data pixels are NaN in any band or, with a
    `nodata_value`, equal to it in all bands (include/drs_hip.h: drs_noise_target_nodata).  valid: (n, 1, H, W) uint8.  At valid
    pixels x_t and target are `noise_images` / `noise_v_target`'s; at no-data pixels x_t is the noised `fill` and target 0."""
    lib = _lib.load()
    x0 = _req(x0, "x0"); eps = _req(eps, "eps"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    if prediction not in PREDICTIONS:
        raise ValueError(f"noise_target_nodata: prediction={prediction!r} must be one of {tuple(PREDICTIONS)}")
    if x0.dim() != 4 or eps.shape != x0.shape:
        raise RuntimeError(f"noise_target_nodata: x0 {tuple(x0.shape)} and eps {tuple(eps.shape)} must be the same (n, C, H, W)")
    n, C_, H, W = x0.shape
    if t.numel() != n:
        raise RuntimeError(f"noise_target_nodata: t has {t.numel()} elements, x0 has {n} images")
    value = math.nan if nodata_value is None else nodata_rule(nodata_value)
    x_t, target = torch.empty_like(x0), torch.empty_like(x0)
    valid = torch.empty((n, 1, H, W), dtype=torch.uint8, device=x0.device)
    with torch.cuda.device(x0.device):
        st = lib.drs_noise_target_nodata(_ptr(x0), _ptr(eps), _ptr(t), _ptr(alpha_hat), alpha_hat.numel(), PREDICTIONS[prediction],
                                         value, float(fill), _ptr(x_t), _ptr(target), _ptr(valid), n, C_, H * W,
                                         _stream(x0.device))
    _lib.check(st, "drs_noise_target_nodata")
    return x_t, target, valid


def threshold_rank(x0_threshold, chw):
    """The 0-based rank k = floor(p (chw - 1)) of the order statistic behind `x0_threshold` = p, 0 < p <= 1, among chw values:
    torch.quantile(..., interpolation="lower")."""
    p = float(x0_threshold)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"x0_threshold={x0_threshold!r} must lie in (0, 1]")
    return min(max(int(math.floor(p * (chw - 1))), 0), max(chw - 1, 0))


_THRESHOLD_WS = {}  # device index -> uint8 workspace of drs_x0_quantile / drs_pred_to_eps_dyn, grown as needed


def _threshold_workspace(lib, n, device):
    need = lib.drs_x0_threshold_workspace_bytes(n)
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _THRESHOLD_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _THRESHOLD_WS[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    return ws


def pred_to_eps_(pred, x, t, alpha_hat, prediction="eps", x0_clip=None, pred_uncond=None, cfg_scale=0.0, out=None,
                 x0_threshold=None, scale_out=None):
    """The network's `pred` (n, ...) - of kind `prediction`: "eps", "v" or "x0" - as the eps the reverse-step wrappers take, in
    place (or into `out`), against the state `x` the network saw at the levels `t` (n int64 values on the device); include/
    drs_hip.h: drs_pred_to_eps.  With `pred_uncond` the prediction is torch.lerp(pred_uncond, pred, cfg_scale) first; with
    `x0_clip=(lo, hi)` the x0 the prediction implies is clamped to that range before eps is formed from it.  Returns eps.
    With `x0_threshold=p` (0 < p <= 1; needs `x0_clip`) the clamp is dynamic thresholding instead (drs_pred_to_eps_dyn): per
    image, s = the floor(p (chw - 1))-th smallest |x0 - centre|; where s exceeds the half-range, x0 is clamped to centre +- s and
    rescaled into the range.  `scale_out`: (n,) fp32, gets every image's s.  `x` must then not share memory with the result."""
    lib = _lib.load()
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction={prediction!r} must be one of {tuple(PREDICTIONS)}")
    if x0_threshold is not None:
        threshold_rank(x0_threshold, 1)  # (ValueError for a p outside (0, 1])
        if x0_clip is None:
            raise ValueError("pred_to_eps_: x0_threshold needs x0_clip=(lo, hi), the range it thresholds to")
    _req_state(pred, "pred_to_eps_", "pred")
    x = _req(x, "x"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    pred_uncond = _req(pred_uncond, "pred_uncond") if pred_uncond is not None else None
    if out is None:
        out = pred
    else:
        _req_state(out, "pred_to_eps_", "out")
    _req_numel("pred_to_eps_", pred, (("x", x), ("pred_uncond", pred_uncond), ("out", out)), "pred")
    n = pred.shape[0] if pred.dim() else 0
    if t.numel() != n:
        raise RuntimeError(f"pred_to_eps_: t has {t.numel()} elements, pred has {n} images")
    flag, lo, hi = _clamp_args(x0_clip, "pred_to_eps_")
    if flag and not lo < hi:
        raise ValueError(f"pred_to_eps_: x0_clip=({lo}, {hi}) needs lo < hi")
    chw = pred.numel() // n if n else 0
    if x0_threshold is not None:
        k = threshold_rank(x0_threshold, chw)
        if scale_out is not None:
            _req_state(scale_out, "pred_to_eps_", "scale_out")
            if scale_out.numel() != n:
                raise RuntimeError(f"pred_to_eps_: scale_out has {scale_out.numel()} elements, pred has {n} images")
        if n == 0 or chw == 0:
            return out
        if x.data_ptr() == out.data_ptr():
            raise RuntimeError("pred_to_eps_: with x0_threshold, x and the result must be two buffers")
        ws = _threshold_workspace(lib, n, pred.device)
        with torch.cuda.device(pred.device):
            st = lib.drs_pred_to_eps_dyn(_ptr(pred), _ptr(pred_uncond), float(cfg_scale), _ptr(x), _ptr(t), _ptr(alpha_hat),
                                         alpha_hat.numel(), PREDICTIONS[prediction], lo, hi, k, _ptr(out), _ptr(scale_out), n,
                                         chw, _ptr(ws), ws.numel(), _stream(pred.device))
        _lib.check(st, "drs_pred_to_eps_dyn")
        return out
    if scale_out is not None:
        raise ValueError("pred_to_eps_: scale_out is written with x0_threshold only")
    with torch.cuda.device(pred.device):
        st = lib.drs_pred_to_eps(_ptr(pred), _ptr(pred_uncond), float(cfg_scale), _ptr(x), _ptr(t), _ptr(alpha_hat),
                                 alpha_hat.numel(), PREDICTIONS[prediction], flag, lo, hi, _ptr(out), n, chw,
                                 _stream(pred.device))
    _lib.check(st, "drs_pred_to_eps")
    return out


def x0_abs_quantile(pred, x, t, alpha_hat, prediction, x0_clip, q, pred_uncond=None, cfg_scale=0.0):
    """(n,) fp32: per image of `pred`, the floor(q (chw - 1))-th smallest |x0 - (lo + hi) / 2| of the x0 the (guided) prediction
    implies - the scale `pred_to_eps_(..., x0_threshold=q)` thresholds with, as found (include/drs_hip.h: drs_x0_quantile).
    An exact order statistic (torch.quantile's interpolation="lower"), all bands ranked together; `pred` is left as it is."""
    lib = _lib.load()
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction={prediction!r} must be one of {tuple(PREDICTIONS)}")
    pred = _req(pred, "pred"); x = _req(x, "x"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    pred_uncond = _req(pred_uncond, "pred_uncond") if pred_uncond is not None else None
    _req_numel("x0_abs_quantile", pred, (("x", x), ("pred_uncond", pred_uncond)), "pred")
    n = pred.shape[0] if pred.dim() else 0
    if t.numel() != n:
        raise RuntimeError(f"x0_abs_quantile: t has {t.numel()} elements, pred has {n} images")
    flag, lo, hi = _clamp_args(x0_clip, "x0_abs_quantile")
    if not flag:
        raise ValueError("x0_abs_quantile: x0_clip=(lo, hi) gives the range and is required")
    if not lo < hi:
        raise ValueError(f"x0_abs_quantile: x0_clip=({lo}, {hi}) needs lo < hi")
    chw = pred.numel() // n if n else 0
    k = threshold_rank(q, chw)
    x0 = torch.empty_like(pred)
    scale = torch.zeros(n, dtype=torch.float32, device=pred.device)
    if n == 0 or chw == 0:
        return scale
    ws = _threshold_workspace(lib, n, pred.device)
    with torch.cuda.device(pred.device):
        st = lib.drs_x0_quantile(_ptr(pred), _ptr(pred_uncond), float(cfg_scale), _ptr(x), _ptr(t), _ptr(alpha_hat),
                                 alpha_hat.numel(), PREDICTIONS[prediction], lo, hi, k, _ptr(x0), _ptr(scale), n, chw, _ptr(ws),
                                 ws.numel(), _stream(pred.device))
    _lib.check(st, "drs_x0_quantile")
    return scale


def timestep_table(noise_steps, n, device):
    """(noise_steps, n) int64: row i is the reference's `t = (torch.ones(n) * i).long()` of sampling step i
    (train_diffusion_superres.py:237) for every step of a chain, built once: a row view per step instead of a fill kernel
    per step (one launch of ~4 us in a 1.35 ms step)."""
    return torch.arange(noise_steps, dtype=torch.int64, device=device).unsqueeze(1).expand(noise_steps, n).contiguous()


def sampler_step_(x, eps_pred, noise, t, alpha, alpha_hat, beta):
    """In-place ancestral update of x for the scalar timestep t (noise may be None)."""
    lib = _lib.load()
    _req_state(x, "sampler_step_")
    eps_pred = _req(eps_pred, "eps_pred")
    noise = _req(noise, "noise") if noise is not None else None
    with torch.cuda.device(x.device):
        st = lib.drs_sampler_step(_ptr(x), _ptr(eps_pred), _ptr(noise), int(t), _ptr(alpha), _ptr(alpha_hat),
                                  _ptr(beta), alpha.numel(), x.numel(), _stream(x.device))
    _lib.check(st, "drs_sampler_step")
    return x


def sampler_step_cfg_(x, eps_cond, eps_uncond, cfg_scale, noise, t, alpha, alpha_hat, beta):
    """In-place ancestral update with eps = torch.lerp(eps_uncond, eps_cond, cfg_scale) folded in
    (reference generate_new_imgs/train_diffusion_generation.py:236-249)."""
    lib = _lib.load()
    _req_state(x, "sampler_step_cfg_")
    eps_cond = _req(eps_cond, "eps_cond")
    eps_uncond = _req(eps_uncond, "eps_uncond")
    noise = _req(noise, "noise") if noise is not None else None
    with torch.cuda.device(x.device):
        st = lib.drs_sampler_step_cfg(_ptr(x), _ptr(eps_cond), _ptr(eps_uncond), float(cfg_scale), _ptr(noise), int(t),
                                      _ptr(alpha), _ptr(alpha_hat), _ptr(beta), alpha.numel(), x.numel(),
                                      _stream(x.device))
    _lib.check(st, "drs_sampler_step_cfg")
    return x


def ddim_step_(x, eps_cond, noise, t, t_prev, eta, alpha_hat, eps_uncond=None, cfg_scale=0.0):
    """In-place DDIM update of x from timestep t to t_prev (include/drs_hip.h: drs_ddim_step); with `eps_uncond` the
    prediction is torch.lerp(eps_uncond, eps_cond, cfg_scale).  `noise` may be None when eta == 0 or t_prev == 0."""
    lib = _lib.load()
    _req_state(x, "ddim_step_")
    eps_cond = _req(eps_cond, "eps_cond")
    eps_uncond = _req(eps_uncond, "eps_uncond") if eps_uncond is not None else None
    noise = _req(noise, "noise") if noise is not None else None
    alpha_hat = _req(alpha_hat, "alpha_hat")
    _req_numel("ddim_step_", x, (("eps_cond", eps_cond), ("eps_uncond", eps_uncond), ("noise", noise)))
    with torch.cuda.device(x.device):
        st = lib.drs_ddim_step(_ptr(x), _ptr(eps_cond), _ptr(eps_uncond), float(cfg_scale), _ptr(noise), int(t),
                               int(t_prev), float(eta), _ptr(alpha_hat), alpha_hat.numel(), x.numel(), _stream(x.device))
    _lib.check(st, "drs_ddim_step")
    return x


def _req_history(op, x, hist, t_q, state="x"):
    """The x0 history of a DPM-Solver++(2M) move: as the state it goes with, used as it is, and memory of its own - the kernels
    take both as __restrict__, so no byte of `hist` may lie inside `state` (a shifted view of one buffer is refused too)."""
    _req_state(hist, op, "hist")
    _req_numel(op, x, (("hist", hist),), state)
    nbytes = x.numel() * x.element_size()
    if hist.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < hist.data_ptr() + nbytes:
        raise RuntimeError(f"{op}: hist must not overlap {state}")
    return -1 if t_q is None else int(t_q)


def dpm_step_(x, eps_cond, hist, t_q, t, t_p, alpha_hat, eps_uncond=None, cfg_scale=0.0):
    """In-place DPM-Solver++(2M) move of x from level t to t_p (include/drs_hip.h: drs_dpm_step); `hist` (as x) receives the x0
    prediction of this move and, when `t_q` - the level the previous move left - is given, supplies that move's: the move is
    then second order.  `t_q` None or -1: first order, `hist` is only written.  Guidance as in `ddim_step_`."""
    lib = _lib.load()
    _req_state(x, "dpm_step_")
    eps_cond = _req(eps_cond, "eps_cond")
    eps_uncond = _req(eps_uncond, "eps_uncond") if eps_uncond is not None else None
    alpha_hat = _req(alpha_hat, "alpha_hat")
    t_q = _req_history("dpm_step_", x, hist, t_q)
    _req_numel("dpm_step_", x, (("eps_cond", eps_cond), ("eps_uncond", eps_uncond)))
    with torch.cuda.device(x.device):
        st = lib.drs_dpm_step(_ptr(x), _ptr(eps_cond), _ptr(eps_uncond), float(cfg_scale), _ptr(hist), t_q, int(t), int(t_p),
                              _ptr(alpha_hat), alpha_hat.numel(), x.numel(), _stream(x.device))
    _lib.check(st, "drs_dpm_step")
    return x


def inpaint_step_(x, eps_cond, noise, known, mask, t, *, alpha_hat, alpha=None, beta=None, t_prev=None, eta=0.0,
                  eps_uncond=None, cfg_scale=0.0):
    """One reverse move of x (n, C, H, W) with known pixels, in place (include/drs_hip.h: drs_inpaint_step): where `mask`
    (uint8, (n, 1 | C, H, W)) is zero the update of `sampler_step_` / `sampler_step_cfg_` (t_prev None: t -> t - 1, needs alpha
    and beta) or of `ddim_step_` (t -> t_prev with eta), elsewhere `known` forward-noised to the level reached with the same
    `noise`, or `known` itself at level 0.  `noise` may be None only when the move ends at level 0."""
    lib = _lib.load()
    _req_state(x, "inpaint_step_")
    if x.dim() != 4:
        raise RuntimeError(f"inpaint_step_: x must be (n, C, H, W), got {tuple(x.shape)}")
    eps_cond = _req(eps_cond, "eps_cond")
    eps_uncond = _req(eps_uncond, "eps_uncond") if eps_uncond is not None else None
    noise = _req(noise, "noise") if noise is not None else None
    known = _req(known, "known")
    mask = _req(mask, "mask", torch.uint8)
    alpha_hat = _req(alpha_hat, "alpha_hat")
    _req_numel("inpaint_step_", x, (("eps_cond", eps_cond), ("eps_uncond", eps_uncond), ("noise", noise), ("known", known)))
    n, C_, H, W = x.shape
    if mask.dim() != 4 or mask.shape[0] != n or tuple(mask.shape[2:]) != (H, W):
        raise RuntimeError(f"inpaint_step_: mask {tuple(mask.shape)} must be ({n}, 1 or {C_}, {H}, {W})")
    ddim = t_prev is not None
    if not ddim:
        alpha = _req(alpha, "alpha"); beta = _req(beta, "beta")
    with torch.cuda.device(x.device):
        st = lib.drs_inpaint_step(_ptr(x), _ptr(eps_cond), _ptr(eps_uncond), float(cfg_scale), _ptr(noise), _ptr(known),
                                  _ptr(mask), n, C_, H, W, int(mask.shape[1]), int(ddim), int(t), int(t_prev) if ddim else 0,
                                  float(eta), _ptr(alpha) if not ddim else _ptr(None), _ptr(alpha_hat),
                                  _ptr(beta) if not ddim else _ptr(None), alpha_hat.numel(), _stream(x.device))
    _lib.check(st, "drs_inpaint_step")
    return x


def renoise_(x, noise, s, t, alpha_hat):
    """In-place forward jump of x from level s to level t > s >= 1 with `noise` (include/drs_hip.h: drs_renoise)."""
    lib = _lib.load()
    _req_state(x, "renoise_")
    noise = _req(noise, "noise")
    alpha_hat = _req(alpha_hat, "alpha_hat")
    _req_numel("renoise_", x, (("noise", noise),))
    with torch.cuda.device(x.device):
        st = lib.drs_renoise(_ptr(x), _ptr(noise), int(s), int(t), _ptr(alpha_hat), alpha_hat.numel(), x.numel(),
                             _stream(x.device))
    _lib.check(st, "drs_renoise")
    return x


def terminal_step_(x, pred, noise, t, t_prev, alpha_hat, prediction, *, eta=0.0, x0_clip=None, scale=None, pred_uncond=None,
                   cfg_scale=0.0, known=None, known_mask=None, hist=None):
    """The reverse move of x (n, C, H, W) from the terminal level t of a zero-terminal-SNR table (alpha_hat[t] == 0) to t_prev,
    in place (include/drs_hip.h: drs_terminal_step).  `pred` is the network's raw output of kind `prediction` ("v" or "x0";
    ValueError for "eps", whose output at that level names no x0), guided with `pred_uncond` / `cfg_scale`; the x0 it names is
    clamped to `x0_clip`, or thresholded with the per-image `scale` ((n,) fp32: `x0_abs_quantile`); `hist`, when given, receives
    that x0 (the history of `dpm_step_`).  x = sqrt(ah_p) x0 + sqrt((1 - ah_p)(1 - eta^2)) x + eta sqrt(1 - ah_p) noise; `noise`
    is needed iff t_prev > 0 and (eta > 0 or there are known pixels).  With `known` / `known_mask` (as `inpaint_step_`) the
    known pixels get exactly `inpaint_step_`'s value.  A t whose alpha_hat is not 0, or levels outside the table, give NaN."""
    lib = _lib.load()
    if prediction not in PREDICTIONS:
        raise ValueError(f"prediction={prediction!r} must be one of {tuple(PREDICTIONS)}")
    if prediction == "eps":
        raise ValueError("terminal_step_: at alpha_hat == 0 an eps prediction is the state itself and names no x0 "
                         "(prediction must be 'v' or 'x0')")
    _req_state(x, "terminal_step_")
    if x.dim() != 4:
        raise RuntimeError(f"terminal_step_: x must be (n, C, H, W), got {tuple(x.shape)}")
    if not 0.0 <= float(eta) <= 1.0:
        raise ValueError(f"terminal_step_: eta={eta} must lie in [0, 1]")
    pred = _req(pred, "pred")
    pred_uncond = _req(pred_uncond, "pred_uncond") if pred_uncond is not None else None
    noise = _req(noise, "noise") if noise is not None else None
    alpha_hat = _req(alpha_hat, "alpha_hat")
    if (known is None) != (known_mask is None):
        raise RuntimeError("terminal_step_: known and known_mask go together")
    n, C_, H, W = x.shape
    mask_channels = 1
    if known is not None:
        known = _req(known, "known")
        known_mask = _req(known_mask, "known_mask", torch.uint8)
        if known_mask.dim() != 4 or known_mask.shape[0] != n or tuple(known_mask.shape[2:]) != (H, W):
            raise RuntimeError(f"terminal_step_: known_mask {tuple(known_mask.shape)} must be ({n}, 1 or {C_}, {H}, {W})")
        mask_channels = int(known_mask.shape[1])
    _req_numel("terminal_step_", x, (("pred", pred), ("pred_uncond", pred_uncond), ("noise", noise), ("known", known)))
    flag, lo, hi = _clamp_args(x0_clip, "terminal_step_")
    if flag and not lo < hi:
        raise ValueError(f"terminal_step_: x0_clip=({lo}, {hi}) needs lo < hi")
    if scale is not None:
        if not flag:
            raise ValueError("terminal_step_: scale needs x0_clip=(lo, hi), the range it thresholds to")
        scale = _req(scale, "scale")
        if scale.numel() != n:
            raise RuntimeError(f"terminal_step_: scale has {scale.numel()} elements, x has {n} images")
    if hist is not None:
        _req_history("terminal_step_", x, hist, None)
    with torch.cuda.device(x.device):
        st = lib.drs_terminal_step(_ptr(x), _ptr(pred), _ptr(pred_uncond), float(cfg_scale), _ptr(noise), _ptr(known),
                                   _ptr(known_mask), mask_channels, PREDICTIONS[prediction], flag, lo, hi, _ptr(scale),
                                   _ptr(hist), n, C_, H, W, int(t), int(t_prev), float(eta), _ptr(alpha_hat), alpha_hat.numel(),
                                   _stream(x.device))
    _lib.check(st, "drs_terminal_step")
    return x


_RESCALE_WS = {}  # device index -> uint8 workspace of drs_cfg_rescale, grown as needed


def _rescale_workspace(lib, n, chw, device):
    need = lib.drs_cfg_rescale_workspace_bytes(n, chw)
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _RESCALE_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _RESCALE_WS[key] = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
    return ws


def cfg_rescale(cond, uncond, cfg_scale, guidance_rescale, out=None):
    """The guided prediction torch.lerp(uncond, cond, cfg_scale) (n, ...) with every image scaled by 1 + phi (std(cond) /
    std(guided) - 1), phi = `guidance_rescale` in [0, 1] (include/drs_hip.h: drs_cfg_rescale; Lin et al. 2024, section 3.4), into
    `out` (which may be `cond`) or a new tensor.  phi == 0 launches nothing of it: the result is the plain torch.lerp."""
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} must lie in [0, 1]")
    cond = _req(cond, "cond"); uncond = _req(uncond, "uncond")
    _req_numel("cfg_rescale", cond, (("uncond", uncond),), "cond")
    if out is not None:
        _req_state(out, "cfg_rescale", "out")
        _req_numel("cfg_rescale", cond, (("out", out),), "cond")
    if phi == 0.0:
        g = torch.lerp(uncond, cond, float(cfg_scale))
        return g if out is None else out.copy_(g.view_as(out))
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(cond)
    n = cond.shape[0] if cond.dim() else 0
    chw = cond.numel() // n if n else 0
    if n == 0 or chw == 0:
        return out
    ws = _rescale_workspace(lib, n, chw, cond.device)
    with torch.cuda.device(cond.device):
        st = lib.drs_cfg_rescale(_ptr(cond), _ptr(uncond), float(cfg_scale), phi, _ptr(out), n, chw, _ptr(ws), ws.numel(),
                                 _stream(cond.device))
    _lib.check(st, "drs_cfg_rescale")
    return out


def reverse_step_(x, eps, noise, t, t_prev, *, alpha, alpha_hat, beta, ddim=False, eta=0.0, eps_uncond=None, cfg_scale=0.0,
                  known=None, known_mask=None, hist=None, t_q=-1):
    """One reverse move t -> t_prev of x, in place, by the wrapper that takes this kind of move: `dpm_step_` with a history
    `hist` (and `t_q`), `inpaint_step_` with `known` / `known_mask`, else `ddim_step_` on a DDIM chain (`ddim`; t_prev and eta
    count there only) and `sampler_step_` / `sampler_step_cfg_` (with `eps_uncond`) on the ancestral one, where t_prev is t - 1."""
    guided = {"eps_uncond": eps_uncond, "cfg_scale": cfg_scale}
    if hist is not None:
        if known is not None or noise is not None:
            raise RuntimeError("reverse_step_: a DPM-Solver++(2M) move takes neither known pixels nor noise")
        return dpm_step_(x, eps, hist, t_q, t, t_prev, alpha_hat, **(guided if eps_uncond is not None else {}))
    if known is not None:
        form = {"t_prev": t_prev, "eta": eta} if ddim else {"alpha": alpha, "beta": beta}
        return inpaint_step_(x, eps, noise, known, known_mask, t, alpha_hat=alpha_hat, **guided, **form)
    if ddim:
        return ddim_step_(x, eps, noise, t, t_prev, eta, alpha_hat, **(guided if eps_uncond is not None else {}))
    if eps_uncond is None:
        return sampler_step_(x, eps, noise, t, alpha, alpha_hat, beta)
    return sampler_step_cfg_(x, eps, eps_uncond, cfg_scale, noise, t, alpha, alpha_hat, beta)


def _req_known(op, known, mask, shape, state):
    """The known image and its mask of a scene-level call: `known` fp32 of `shape` = (C, H, W), `mask` uint8 (1 | C, H, W), both
    on the device of `state` and given together; (known, mask), contiguous."""
    if (known is None) != (mask is None):
        raise RuntimeError(f"{op}: known and known_mask go together, got " +
                           ("known without known_mask" if mask is None else "known_mask without known"))
    known = _req(known, "known")
    mask = _req(mask, "known_mask", torch.uint8)
    C_, H, W = shape
    if known.device != state.device or mask.device != state.device:
        raise RuntimeError(f"{op}: known is on {known.device}, known_mask on {mask.device}, the scene on {state.device}")
    if tuple(known.shape) != (C_, H, W):
        raise RuntimeError(f"{op}: known {tuple(known.shape)} must be {(C_, H, W)}")
    if mask.dim() != 3 or mask.shape[0] not in (1, C_) or tuple(mask.shape[1:]) != (H, W):
        raise RuntimeError(f"{op}: known_mask {tuple(mask.shape)} must be (1 or {C_}, {H}, {W})")
    return known, mask


_ORIGIN_TABLES = {}  # (origins, device) -> (n, 2) int32 device table, kept for the life of the process (8 bytes per tile)


def _origin_table(origins, device):
    """[(y0, x0), ...] as an (n, 2) int32 table on `device`, uploaded once per layout and device: an upload from pageable
    memory makes the host wait for everything enqueued on the caller's stream, and a tiler asks for the same table every chain.
    The table is shared and READ-ONLY: kernels of any stream may be reading it, so it is never written, freed or evicted."""
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (tuple((int(y), int(x)) for y, x in origins), device)
    table = _ORIGIN_TABLES.get(key)
    if table is None:
        table = _ORIGIN_TABLES[key] = torch.tensor(key[0], dtype=torch.int32).reshape(-1, 2).to(device)
    return table


def aggregate_tiles(tiles, origins, weight, height, width, clamp=(0.0, 1.0), known=None, known_mask=None):
    """Gaussian-weighted blend of (n,C,S,S) tiles placed at `origins` [(y0, x0), ...] into a (C,height,width) image,
    normalised by the summed weights and clamped to [0,1] (reference Aggregation_Sampling.py:90-116).
    Raises like the reference's `assert torch.all(pixel_count != 0)` when a pixel is covered by no tile.
    `clamp=(lo, hi)` clamps to another range and `clamp=None` not at all; `known` (C,height,width) with `known_mask` (uint8,
    (1 | C,height,width), nonzero = known) writes those pixels as `known`, clamped like the rest (include/drs_hip.h:
    drs_aggregate_tiles_known; the default arguments call drs_aggregate_tiles)."""
    lib = _lib.load()
    tiles = _req(tiles, "tiles")
    weight = _req(weight, "weight")
    n, C, S, S2 = tiles.shape
    if S != S2 or tuple(weight.shape) != (S, S) or len(origins) != n:
        raise RuntimeError(f"aggregate_tiles: tiles {tuple(tiles.shape)}, weight {tuple(weight.shape)}, {len(origins)} origins")
    flag, lo, hi = _clamp_args(clamp, "aggregate_tiles")
    plain = known is None and known_mask is None and (flag, lo, hi) == (1, 0.0, 1.0)
    if known is not None or known_mask is not None:
        known, known_mask = _req_known("aggregate_tiles", known, known_mask, (C, int(height), int(width)), tiles)
    org = _origin_table(origins, tiles.device)
    out = torch.empty((C, int(height), int(width)), dtype=torch.float32, device=tiles.device)
    uncovered = torch.zeros(1, dtype=torch.int32, device=tiles.device)
    with torch.cuda.device(tiles.device):
        if plain:
            st = lib.drs_aggregate_tiles(_ptr(tiles), _ptr(org), _ptr(weight), _ptr(out), _ptr(uncovered), n, C, S,
                                         int(height), int(width), _stream(tiles.device))
            _lib.check(st, "drs_aggregate_tiles")
        else:
            st = lib.drs_aggregate_tiles_known(_ptr(tiles), _ptr(org), _ptr(weight), _ptr(known), _ptr(known_mask), _ptr(out),
                                               _ptr(uncovered), n, C, S, int(height), int(width),
                                               int(known_mask.shape[0]) if known_mask is not None else 1, flag, lo, hi,
                                               _stream(tiles.device))
            _lib.check(st, "drs_aggregate_tiles_known")
    if int(uncovered.item()) != 0:
        raise AssertionError("aggregation: some output pixels are covered by no tile (pixel_count == 0)")
    return out


def tile_origins(origins, S, height, width, device):
    """The (n, 2) int32 device table of tile origins [(y0, x0), ...] that `gather_tiles` / `blend_step_` take, checked on
    the host (every window inside the (height, width) scene) and uploaded ONCE per chain, not per step."""
    org = torch.tensor([[int(y), int(x)] for y, x in origins], dtype=torch.int32).reshape(-1, 2)
    if org.shape[0] == 0:
        raise RuntimeError("tile_origins: no tiles")
    if int(org.min()) < 0 or int(org[:, 0].max()) + S > height or int(org[:, 1].max()) + S > width:
        raise RuntimeError(f"tile_origins: a {S}x{S} tile window leaves the {height}x{width} scene")
    return _origin_table(origins, torch.device(device)).clone()  # (the caller's own: a device copy of the shared table)


def _req_origins(origins, name):
    origins = _req(origins, name, torch.int32)
    if origins.dim() != 2 or origins.shape[1] != 2 or origins.shape[0] < 1:
        raise RuntimeError(f"{name} must be an (n, 2) int32 device table (hip_ops.tile_origins), got {tuple(origins.shape)}")
    return origins


def gather_tiles(scene, origins, S, out=None, first=0, count=None):
    """tiles[k] = scene[:, y0:y0+S, x0:x0+S] for the `count` tiles from index `first` of the device table `origins`
    (`tile_origins`), bit-exact: (count, C, S, S), written into `out` when given.  A chunk that runs past the last tile
    repeats it (the padding of a fixed-size chunk of tiles)."""
    lib = _lib.load()
    scene = _req(scene, "scene")
    origins = _req_origins(origins, "origins")
    if scene.dim() != 3:
        raise RuntimeError(f"gather_tiles: scene must be (C, H, W), got {tuple(scene.shape)}")
    C_, Hs, Ws = scene.shape
    n = origins.shape[0]
    count = n - first if count is None else int(count)
    if out is None:
        out = torch.empty((count, C_, S, S), dtype=torch.float32, device=scene.device)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32) or out.numel() != count * C_ * S * S:
        raise RuntimeError(f"gather_tiles: out must be a contiguous fp32 ROCm tensor of {count * C_ * S * S} elements")
    with torch.cuda.device(scene.device):
        st = lib.drs_gather_tiles(_ptr(scene), _ptr(origins), _ptr(out), int(first), count, n, C_, int(S), Hs, Ws,
                                  _stream(scene.device))
    _lib.check(st, "drs_gather_tiles")
    return out


def blend_step_(scene, eps_tiles, origins, weight, noise, t, *, alpha_hat, alpha=None, beta=None, t_prev=None, eta=0.0,
                uncovered=None, hist=None, t_q=-1, known=None, known_mask=None):
    """One reverse step of the scene state (C, H, W), in place, from the noise predictions `eps_tiles` (n, C, S, S) of
    its tiles (only the first n = len(origins) tiles of a longer buffer are read): Gaussian-weighted mean of the covering
    tiles' eps in tile order, then the update of `sampler_step_` (t_prev None: needs alpha and beta) or of `ddim_step_`
    (t -> t_prev with eta).  `noise` (scene shape) may be None as for those.  `uncovered`: optional int32 device counter
    that is increased by the number of pixels no tile covers (include/drs_hip.h: drs_blend_step).  With `hist` (scene shape) the
    update is that of `dpm_step_` from t to t_prev, `t_q` as there; it takes no noise (drs_blend_step_dpm).
    With `known` (scene shape, used as given) and `known_mask` (uint8, (1 | C, H, W), nonzero = known) the step is followed by
    the select of `inpaint_step_` in the same launch: the masked elements become `known` forward-noised to the level reached
    with the same `noise`, or `known` itself at level 0, the others are the step's, bit for bit.  `noise` may then be None
    only when the move ends at level 0; a DPM-Solver++(2M) move keeps no known pixels (drs_blend_step_known)."""
    lib = _lib.load()
    _req_state(scene, "blend_step_", "scene")
    eps_tiles = _req(eps_tiles, "eps_tiles")
    origins = _req_origins(origins, "origins")
    weight = _req(weight, "weight")
    noise = _req(noise, "noise") if noise is not None else None
    alpha_hat = _req(alpha_hat, "alpha_hat")
    if scene.dim() != 3 or eps_tiles.dim() != 4:
        raise RuntimeError(f"blend_step_: scene {tuple(scene.shape)} must be (C, H, W), eps_tiles {tuple(eps_tiles.shape)} "
                           "(n, C, S, S)")
    C_, Hs, Ws = scene.shape
    n = origins.shape[0]
    S = eps_tiles.shape[2]
    if eps_tiles.shape[0] < n or eps_tiles.shape[1] != C_ or eps_tiles.shape[3] != S or tuple(weight.shape) != (S, S):
        raise RuntimeError(f"blend_step_: eps_tiles {tuple(eps_tiles.shape)}, weight {tuple(weight.shape)}, {n} origins, "
                           f"scene {tuple(scene.shape)}")
    _req_numel("blend_step_", scene, (("noise", noise),), "scene")
    if uncovered is not None:
        uncovered = _req(uncovered, "uncovered", torch.int32)
    if hist is not None:
        if noise is not None or t_prev is None:
            raise RuntimeError("blend_step_: a DPM-Solver++(2M) move (hist) needs t_prev and takes no noise")
        t_q = _req_history("blend_step_", scene, hist, t_q, "scene")
    if known is not None or known_mask is not None:
        if hist is not None:
            raise RuntimeError("blend_step_: a DPM-Solver++(2M) move (hist) keeps no known pixels")
        known, known_mask = _req_known("blend_step_", known, known_mask, (C_, Hs, Ws), scene)
    with torch.cuda.device(scene.device):
        if known is not None:
            ddim = t_prev is not None
            if not ddim:
                alpha = _req(alpha, "alpha"); beta = _req(beta, "beta")
            st = lib.drs_blend_step_known(_ptr(scene), _ptr(eps_tiles), _ptr(origins), _ptr(weight), _ptr(noise), _ptr(known),
                                          _ptr(known_mask), _ptr(uncovered), n, C_, S, Hs, Ws, int(known_mask.shape[0]), int(ddim),
                                          int(t), int(t_prev) if ddim else 0, float(eta), _ptr(alpha) if not ddim else _ptr(None),
                                          _ptr(alpha_hat), _ptr(beta) if not ddim else _ptr(None), alpha_hat.numel(),
                                          _stream(scene.device))
            _lib.check(st, "drs_blend_step_known")
        elif hist is not None:
            st = lib.drs_blend_step_dpm(_ptr(scene), _ptr(eps_tiles), _ptr(origins), _ptr(weight), _ptr(hist), _ptr(uncovered),
                                        n, C_, S, Hs, Ws, t_q, int(t), int(t_prev), _ptr(alpha_hat), alpha_hat.numel(),
                                        _stream(scene.device))
            _lib.check(st, "drs_blend_step_dpm")
        elif t_prev is None:
            alpha = _req(alpha, "alpha"); beta = _req(beta, "beta")
            st = lib.drs_blend_step(_ptr(scene), _ptr(eps_tiles), _ptr(origins), _ptr(weight), _ptr(noise), _ptr(uncovered),
                                    n, C_, S, Hs, Ws, int(t), _ptr(alpha), _ptr(alpha_hat), _ptr(beta), alpha_hat.numel(),
                                    _stream(scene.device))
            _lib.check(st, "drs_blend_step")
        else:
            st = lib.drs_blend_step_ddim(_ptr(scene), _ptr(eps_tiles), _ptr(origins), _ptr(weight), _ptr(noise),
                                         _ptr(uncovered), n, C_, S, Hs, Ws, int(t), int(t_prev), float(eta), _ptr(alpha_hat),
                                         alpha_hat.numel(), _stream(scene.device))
            _lib.check(st, "drs_blend_step_ddim")
    return scene


def _req_image_pair(sr, hr, what):
    sr = _req(sr, "sr"); hr = _req(hr, "hr")
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise RuntimeError(f"{what}: sr {tuple(sr.shape)} and hr {tuple(hr.shape)} must be the same (B, C, H, W)")
    if hr.device != sr.device:
        raise RuntimeError(f"{what}: sr is on {sr.device}, hr on {hr.device}")
    return sr, hr


def metrics_workspace(B, C, H, W, device):
    """The scratch buffer `metrics_pointwise` and `ssim_mean` take (either call, stream-ordered)."""
    return torch.empty(max(_lib.load().drs_metrics_workspace_bytes(B, C, H, W), 8), dtype=torch.uint8, device=device)


def metrics_nodata_workspace(B, C, H, W, device):
    """The scratch buffer `metrics_pointwise_nodata` and `ssim_nodata` take (either call, stream-ordered)."""
    return torch.empty(max(_lib.load().drs_metrics_nodata_workspace_bytes(B, C, H, W), 8), dtype=torch.uint8, device=device)


def _metrics_launch(entry, what, sr, hr, width, clamp, workspace, masked=False, nodata=None):
    """One call of the C-ABI `entry` ("drs_metrics_pointwise" | "drs_ssim") into a fresh (B, *width(C)) float64 tensor, or -
    `masked` - of its `_nodata` sibling, which takes the `nodata` rule's value after hr and the larger workspace."""
    lib = _lib.load()
    sr, hr = _req_image_pair(sr, hr, what)
    rule = (nodata_rule(nodata),) if masked else ()
    B, C_, H, W = sr.shape
    if workspace is None:
        ws = (metrics_nodata_workspace if masked else metrics_workspace)(B, C_, H, W, sr.device)
    else:
        ws = _req(workspace, "workspace", torch.uint8)
    out = torch.empty((B, *width(C_)), dtype=torch.float64, device=sr.device)
    entry += "_nodata" if masked else ""
    with torch.cuda.device(sr.device):
        st = getattr(lib, entry)(_ptr(sr), _ptr(hr), *rule, _ptr(out), B, C_, H, W, int(bool(clamp)), _ptr(ws), ws.numel(),
                                 _stream(sr.device))
    _lib.check(st, entry)
    return out


def metrics_pointwise(sr, hr, clamp=True, workspace=None):
    """Per-image sums of one pass over sr and hr (B, C, H, W): a (B, 2 C + 2) float64 device tensor holding the per-band
    squared error, the per-band sum of hr, the sum of the per-pixel spectral angles in radians and the number of pixels in
    that sum (include/drs_hip.h: drs_metrics_pointwise)."""
    return _metrics_launch("drs_metrics_pointwise", "metrics_pointwise", sr, hr, lambda C_: (2 * C_ + 2,), clamp, workspace)


def ssim_mean(sr, hr, clamp=True, workspace=None):
    """Per-image mean SSIM over bands and valid window positions: a (B,) float64 device tensor (include/drs_hip.h: drs_ssim)."""
    return _metrics_launch("drs_ssim", "ssim_mean", sr, hr, lambda C_: (), clamp, workspace)


def metrics_pointwise_nodata(sr, hr, nodata, clamp=True, workspace=None):
    """`metrics_pointwise` over the valid pixels of hr (`nodata`: True / "nan" or the no-data value): a (B, 2 C + 3) float64
    device tensor, the last column the number of valid pixels (include/drs_hip.h: drs_metrics_pointwise_nodata)."""
    return _metrics_launch("drs_metrics_pointwise", "metrics_pointwise_nodata", sr, hr, lambda C_: (2 * C_ + 3,), clamp, workspace,
                           masked=True, nodata=nodata)


def ssim_nodata(sr, hr, nodata, clamp=True, workspace=None):
    """Per image (mean SSIM over bands and over the window positions whose 11 x 11 pixels of hr are all valid - NaN when there
    is none -, number of such positions): a (B, 2) float64 device tensor (include/drs_hip.h: drs_ssim_nodata)."""
    return _metrics_launch("drs_ssim", "ssim_nodata", sr, hr, lambda C_: (2,), clamp, workspace, masked=True, nodata=nodata)


def _req_members(members, what, truth=None):
    """The (N, B, C, H, W) members (and the truth) of an ensemble call.  Unlike the other wrappers these refuse a
    non-contiguous tensor instead of copying it: the members are N times an image batch."""
    for t, name in ((members, "members"), (truth, "truth"))[:1 if truth is None else 2]:
        _req(t, name)
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} {tuple(t.shape)} with strides {t.stride()} must be contiguous")
    if members.dim() != 5 or not 2 <= members.shape[0] <= 32:
        raise RuntimeError(f"{what}: members {tuple(members.shape)} must be (N, B, C, H, W) with 2 <= N <= 32")
    return members


def _clamp_args(clamp, what):
    """(flag, lo, hi) of a `clamp=None | (lo, hi)` argument."""
    if clamp is None:
        return 0, 0.0, 0.0
    lo, hi = (float(v) for v in clamp)
    if not lo <= hi:
        raise ValueError(f"{what}: clamp=({lo}, {hi}) needs lo <= hi")
    return 1, lo, hi


def ensemble_stats(members, quantiles=None, clamp=None, mean=True, std=True):
    """Per-element statistics over the member axis of `members` (N, B, C, H, W), 2 <= N <= 32: (mean, std, quantiles) as
    (B, C, H, W), (B, C, H, W) and (Q, B, C, H, W) fp32 device tensors from one pass over the members (include/drs_hip.h:
    drs_ensemble_stats).  `quantiles`: up to 8 values in [0, 1] (None: no quantile map, an empty list: an empty tensor);
    `clamp=(lo, hi)` clamps the members first; `mean=False` / `std=False` leave that map out (None in its place)."""
    lib = _lib.load()
    members = _req_members(members, "ensemble_stats")
    N, shape = members.shape[0], tuple(members.shape[1:])
    flag, lo, hi = _clamp_args(clamp, "ensemble_stats")
    qs = [float(v) for v in quantiles] if quantiles is not None else []
    if len(qs) > 8 or any(not 0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"ensemble_stats: quantiles {qs} must be at most 8 values in [0, 1]")
    mean_t = torch.empty(shape, dtype=torch.float32, device=members.device) if mean else None
    std_t = torch.empty(shape, dtype=torch.float32, device=members.device) if std else None
    q_t = torch.empty((len(qs),) + shape, dtype=torch.float32, device=members.device) if quantiles is not None else None
    q_arr = (C.c_double * max(len(qs), 1))(*qs)
    with torch.cuda.device(members.device):
        st = lib.drs_ensemble_stats(_ptr(members), _ptr(mean_t), _ptr(std_t), _ptr(q_t) if qs else None,
                                    C.cast(q_arr, C.c_void_p), len(qs), N, *shape, flag, lo, hi, _stream(members.device))
    _lib.check(st, "drs_ensemble_stats")
    return mean_t, std_t, q_t


def ensemble_scores(members, truth, clamp=None, crps_map=False):
    """Scores of `members` (N, B, C, H, W) against `truth` (B, C, H, W): (sums, rank_histogram, crps) = a (B, 3) float64 tensor
    of the per-image sums over C, H, W of the CRPS, of the unbiased member variance and of (mean - truth)^2, the (B, N + 1)
    int64 counts of the elements by the rank of the truth among the members, and the (B, C, H, W) fp32 CRPS map (None
    without `crps_map`); include/drs_hip.h: drs_ensemble_scores.  `clamp=(lo, hi)` clamps members and truth first."""
    lib = _lib.load()
    members = _req_members(members, "ensemble_scores", truth)
    if tuple(truth.shape) != tuple(members.shape[1:]):
        raise RuntimeError(f"ensemble_scores: truth {tuple(truth.shape)} must be the members' {tuple(members.shape[1:])}")
    if truth.device != members.device:
        raise RuntimeError(f"ensemble_scores: members are on {members.device}, truth on {truth.device}")
    N, (B, C_, H, W) = members.shape[0], truth.shape
    flag, lo, hi = _clamp_args(clamp, "ensemble_scores")
    ws = torch.empty(max(lib.drs_ensemble_workspace_bytes(N, B, C_, H, W), 8), dtype=torch.uint8, device=members.device)
    sums = torch.empty((B, 3), dtype=torch.float64, device=members.device)
    hist = torch.empty((B, N + 1), dtype=torch.int64, device=members.device)
    crps = torch.empty_like(truth) if crps_map else None
    with torch.cuda.device(members.device):
        st = lib.drs_ensemble_scores(_ptr(members), _ptr(truth), _ptr(crps), _ptr(sums), _ptr(hist), N, B, C_, H, W, flag, lo,
                                     hi, _ptr(ws), ws.numel(), _stream(members.device))
    _lib.check(st, "drs_ensemble_scores")
    return sums, hist, crps


def _req_colorfix(sr, guide, what):
    """The (B, C, H, W) pair of a colour-correction call.  Like the ensemble wrappers these refuse a non-contiguous tensor
    instead of copying it."""
    for t, name in ((sr, "sr"), (guide, "guide")):
        _req(t, name)
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} {tuple(t.shape)} with strides {t.stride()} must be contiguous")
    if sr.dim() != 4 or sr.shape != guide.shape:
        raise RuntimeError(f"{what}: sr {tuple(sr.shape)} and guide {tuple(guide.shape)} must be the same (B, C, H, W)")
    if guide.device != sr.device:
        raise RuntimeError(f"{what}: sr is on {sr.device}, guide on {guide.device}")


def colorfix_wavelet(sr, guide, levels=5):
    """sr + low(guide - sr) per plane of (B, C, H, W), `low` = `levels` (1 .. 5) dilated 3 x 3 binomial blurs on replicate
    padding: the sample's detail on the guide's large-scale content (include/drs_hip.h: drs_colorfix_wavelet)."""
    lib = _lib.load()
    _req_colorfix(sr, guide, "colorfix_wavelet")
    out = torch.empty_like(sr)
    with torch.cuda.device(sr.device):
        st = lib.drs_colorfix_wavelet(_ptr(sr), _ptr(guide), _ptr(out), *sr.shape, int(levels), _stream(sr.device))
    _lib.check(st, "drs_colorfix_wavelet")
    return out


def colorfix_adain(sr, guide):
    """a sr + b per plane of (B, C, H, W), with the plane's mean and unbiased standard deviation moved onto the guide's
    (include/drs_hip.h: drs_colorfix_adain)."""
    lib = _lib.load()
    _req_colorfix(sr, guide, "colorfix_adain")
    out = torch.empty_like(sr)
    ws = torch.empty(max(lib.drs_colorfix_adain_workspace_bytes(*sr.shape), 8), dtype=torch.uint8, device=sr.device)
    with torch.cuda.device(sr.device):
        st = lib.drs_colorfix_adain(_ptr(sr), _ptr(guide), _ptr(out), *sr.shape, _ptr(ws), ws.numel(), _stream(sr.device))
    _lib.check(st, "drs_colorfix_adain")
    return out


_SEP_WS = {}  # device index -> uint8 workspace of drs_sep_apply / drs_sep_project / drs_sep_project_eps, grown as needed


def _sep_workspace(lib, shape, device):
    need = lib.drs_sep_workspace_bytes(*shape)
    key = device.index if device.index is not None else torch.cuda.current_device()
    ws = _SEP_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _SEP_WS[key] = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    return ws


def _req_sep(op, x, name="x"):
    x = _req(x, name)
    if x.dim() != 4 or min(x.shape) < 1:
        raise RuntimeError(f"{op}: {name} must be a (B, C, H, W) tensor without an empty extent, got {tuple(x.shape)}")
    return x


def _req_matrix(op, m, name, shape):
    m = _req(m, name)
    if tuple(m.shape) != tuple(shape):
        raise RuntimeError(f"{op}: {name} is {tuple(m.shape)}, expected {tuple(shape)}")
    return m




def _band_table(op, band_op, n_ops, Cn):
    """The host int32 table the *_bands entries take: `band_op` (Cn slots in 0 .. n_ops - 1), or None for the entries' default."""
    if not 1 <= n_ops <= Cn:
        raise RuntimeError(f"{op}: {n_ops} operators for {Cn} bands (need 1 .. the band count)")
    if band_op is None:
        return None
    band_op = [int(b) for b in band_op]
    if len(band_op) != Cn or min(band_op) < 0 or max(band_op) >= n_ops:
        raise RuntimeError(f"{op}: band_op={band_op} must name one of the {n_ops} operators for each of the {Cn} bands")
    return (C.c_int32 * Cn)(*band_op)


def sep_apply(x, d_y, d_x, band_op=None):
    """d_y x d_x^T per plane of x (B, C, H, W) for matrices d_y (h, H) and d_x (w, W): (B, C, h, w), exact fp32 products in a
    fixed order (include/drs_hip.h: drs_sep_apply).  Stacked matrices (n_ops, h, H) / (n_ops, w, W): band b takes the pair
    band_op[b] (None: min(b, n_ops - 1); drs_sep_apply_bands)."""
    lib = _lib.load()
    x = _req_sep("sep_apply", x)
    B, Cn, H, W = x.shape
    d_y, d_x = _req(d_y, "d_y"), _req(d_x, "d_x")
    if d_y.dim() != d_x.dim() or d_y.dim() not in (2, 3) or d_y.shape[-1] != H or d_x.shape[-1] != W or (
            d_y.dim() == 3 and d_y.shape[0] != d_x.shape[0]):
        raise RuntimeError(f"sep_apply: d_y {tuple(d_y.shape)} / d_x {tuple(d_x.shape)} do not take {H} x {W} planes")
    if d_y.dim() == 2 and band_op is not None:
        raise RuntimeError("sep_apply: band_op goes with stacked (n_ops, ., .) matrices")
    h, w = d_y.shape[-2], d_x.shape[-2]
    table = _band_table("sep_apply", band_op, d_y.shape[0], Cn) if d_y.dim() == 3 else None
    out = torch.empty((B, Cn, h, w), dtype=torch.float32, device=x.device)
    ws = _sep_workspace(lib, (B, Cn, H, W, h, w), x.device)
    with torch.cuda.device(x.device):
        if d_y.dim() == 2:
            st = lib.drs_sep_apply(_ptr(x), _ptr(d_y), _ptr(d_x), _ptr(out), B, Cn, H, W, h, w, _ptr(ws), ws.numel(),
                                   _stream(x.device))
        else:
            st = lib.drs_sep_apply_bands(_ptr(x), _ptr(d_y), _ptr(d_x), _ptr(out), B, Cn, H, W, h, w, table, d_y.shape[0],
                                         _ptr(ws), ws.numel(), _stream(x.device))
    _lib.check(st, "drs_sep_apply" if d_y.dim() == 2 else "drs_sep_apply_bands")
    return out


def _sep_projector_args(op, projector, yt, B, Cn, H, W):
    """(yt, the five matrices, h, w, bands): `bands` None for a one-operator projector (2-D matrices: the plain entries), else
    (the host table or None, n_ops) of a stacked one."""
    stacked = projector.D_y.dim() == 3
    lead = (projector.D_y.shape[0],) if stacked else ()
    h, w = projector.D_y.shape[-2], projector.D_x.shape[-2]
    mats = (_req_matrix(op, projector.D_y, "D_y", lead + (h, H)), _req_matrix(op, projector.D_x, "D_x", lead + (w, W)),
            _req_matrix(op, projector.U_y, "U_y", lead + (H, h)), _req_matrix(op, projector.U_x, "U_x", lead + (W, w)),
            _req_matrix(op, projector.G, "G", lead + (h, w)))
    yt = _req_matrix(op, yt, "yt", (B, Cn, h, w))
    bands = (_band_table(op, getattr(projector, "band_op", None), lead[0], Cn), lead[0]) if stacked else None
    return yt, mats, h, w, bands


def sep_project(x, yt, projector, strength=1.0, out=None):
    """x + strength U_y (G o (yt - D_y x D_x^T)) U_x^T per plane of x (B, C, H, W), with the tensors of `projector` (a
    consistency.LRProjector) and yt = projector.prepare(y); into `out` (may be x; default: a new tensor).  include/drs_hip.h:
    drs_sep_project, or drs_sep_project_bands for the stacked tensors of a per-band projector."""
    lib = _lib.load()
    x = _req_sep("sep_project", x)
    B, Cn, H, W = x.shape
    yt, mats, h, w, bands = _sep_projector_args("sep_project", projector, yt, B, Cn, H, W)
    if out is None:
        out = torch.empty_like(x)
    else:
        _req_state(out, "sep_project", "out")
        _req_numel("sep_project", x, (("out", out),))
    ws = _sep_workspace(lib, (B, Cn, H, W, h, w), x.device)
    with torch.cuda.device(x.device):
        if bands is None:
            st = lib.drs_sep_project(_ptr(x), _ptr(yt), *(_ptr(m) for m in mats), float(strength), _ptr(out), B, Cn, H, W, h, w,
                                     _ptr(ws), ws.numel(), _stream(x.device))
        else:
            st = lib.drs_sep_project_bands(_ptr(x), _ptr(yt), *(_ptr(m) for m in mats), float(strength), _ptr(out), B, Cn, H, W,
                                           h, w, *bands, _ptr(ws), ws.numel(), _stream(x.device))
    _lib.check(st, "drs_sep_project" if bands is None else "drs_sep_project_bands")
    return out


def lr_consistent_eps_(eps, x, t, alpha_hat, yt, projector, strength=1.0):
    """The in-chain projection, in place on `eps` (B, C, H, W): the noise prediction of the x0 that `eps` implies for the state
    `x` at the levels `t` (B int64 values on the device), moved onto the images `projector`'s operator maps to the observation
    behind yt = projector.prepare(y).  x0 is formed as it is loaded and never stored; strength 0 leaves eps its bits
    (include/drs_hip.h: drs_sep_project_eps, or drs_sep_project_eps_bands for a per-band projector).  Returns eps."""
    lib = _lib.load()
    _req_state(eps, "lr_consistent_eps_", "eps")
    if eps.dim() != 4 or min(eps.shape) < 1:
        raise RuntimeError(f"lr_consistent_eps_: eps must be a (B, C, H, W) tensor without an empty extent, got {tuple(eps.shape)}")
    x = _req(x, "x"); t = _req(t, "t", torch.int64); alpha_hat = _req(alpha_hat, "alpha_hat")
    if tuple(x.shape) != tuple(eps.shape):
        raise RuntimeError(f"lr_consistent_eps_: x is {tuple(x.shape)}, eps {tuple(eps.shape)}")
    B, Cn, H, W = eps.shape
    if t.numel() != B:
        raise RuntimeError(f"lr_consistent_eps_: t has {t.numel()} elements, eps has {B} images")
    yt, mats, h, w, bands = _sep_projector_args("lr_consistent_eps_", projector, yt, B, Cn, H, W)
    ws = _sep_workspace(lib, (B, Cn, H, W, h, w), eps.device)
    with torch.cuda.device(eps.device):
        if bands is None:
            st = lib.drs_sep_project_eps(_ptr(eps), _ptr(x), _ptr(t), _ptr(alpha_hat), alpha_hat.numel(), _ptr(yt),
                                         *(_ptr(m) for m in mats), float(strength), B, Cn, H, W, h, w, _ptr(ws), ws.numel(),
                                         _stream(eps.device))
        else:
            st = lib.drs_sep_project_eps_bands(_ptr(eps), _ptr(x), _ptr(t), _ptr(alpha_hat), alpha_hat.numel(), _ptr(yt),
                                               *(_ptr(m) for m in mats), float(strength), B, Cn, H, W, h, w, *bands, _ptr(ws),
                                               ws.numel(), _stream(eps.device))
    _lib.check(st, "drs_sep_project_eps" if bands is None else "drs_sep_project_eps_bands")
    return eps


def fir_decimate(x, taps_y, taps_x, left, m, band_op=None, noise=None, sigma=None, clamp=False):
    """The separable FIR blur and decimation by m of x (B, C, H, W) -> (B, C, H // m, W // m): LR pixel (i, j) of band b sums
    taps_y[op][u] taps_x[op][v] x[clamp(i m + u - Ly)][clamp(j m + v - Lx)], op = band_op[b] (None: min(b, n_ops - 1)), over the
    rows of taps_y (n_ops, ntaps_y) / taps_x (n_ops, ntaps_x) (1-D: one operator); `left` = L or (Ly, Lx).  noise (B, C, h, w)
    standard normals with sigma (C,): + sigma[b] z; clamp: into [0, 1] last.  One launch (include/drs_hip.h: drs_fir_decimate)."""
    lib = _lib.load()
    x = _req_sep("fir_decimate", x)
    B, Cn, H, W = x.shape
    taps_y, taps_x = _req(taps_y, "taps_y"), _req(taps_x, "taps_x")
    if taps_y.dim() == 1 and taps_x.dim() == 1:
        taps_y, taps_x = taps_y[None], taps_x[None]
    if taps_y.dim() != 2 or taps_x.dim() != 2 or taps_y.shape[0] != taps_x.shape[0] or min(taps_y.shape + taps_x.shape) < 1:
        raise RuntimeError(f"fir_decimate: taps_y {tuple(taps_y.shape)} / taps_x {tuple(taps_x.shape)} must be (n_ops, ntaps) each")
    Ly, Lx = (int(left), int(left)) if not isinstance(left, (tuple, list)) else (int(left[0]), int(left[1]))
    m = int(m)
    if m < 1 or H // m < 1 or W // m < 1:
        raise RuntimeError(f"fir_decimate: m={m} leaves no pixel of {H} x {W} planes")
    h, w = H // m, W // m
    table = _band_table("fir_decimate", band_op, taps_y.shape[0], Cn)
    if (noise is None) != (sigma is None):
        raise RuntimeError("fir_decimate: noise and sigma go together")
    if noise is not None:
        noise, sigma = _req_matrix("fir_decimate", noise, "noise", (B, Cn, h, w)), _req_matrix("fir_decimate", sigma, "sigma", (Cn,))
    out = torch.empty((B, Cn, h, w), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = lib.drs_fir_decimate(_ptr(x), _ptr(taps_y), _ptr(taps_x), table, taps_y.shape[0], taps_y.shape[1], taps_x.shape[1],
                                  Ly, Lx, m, _ptr(noise), _ptr(sigma), int(bool(clamp)), _ptr(out), B, Cn, H, W, h, w,
                                  _stream(x.device))
    _lib.check(st, "drs_fir_decimate")
    return out
