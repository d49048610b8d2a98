"""LR-consistent super-resolution: the damped range-null-space projection of an image onto the images a separable linear
degradation maps to the observation (DDNM, Wang et al. 2023; not in the reference).

`SeparableOperator` holds the two float64 matrices of x -> A_y x A_x^T - `downblur` is the trainer's degradation without its
roundings - and makes an `LRProjector`, whose fp32 device tensors the kernels of csrc/consistency.hip take (`degrade`, `project`,
`lr_rmse` here; `hip_ops.lr_consistent_eps_` inside a chain).  `LRConsistency` is the request a `Diffusion`, the tiler and
`evaluate` take; `chain_projector` resolves it for a chain.  `BandOperator` is one `SeparableOperator` per band - the sensor-MTF
degradation's (`SeparableOperator.mtf`, mtf.py) - with the same surface and stacked device tensors."""
import math
import numbers

import numpy as np
import torch

from . import hip_ops

MAX_CONDITION = 1e6  # per axis: beyond it an undamped projector is refused


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def resample_matrix(in_size, out_size):
    """(out_size, in_size) float64: Pillow's antialiased bicubic resampling of one axis (Resample.c: support 2 * scale around
    (i + 0.5) * scale, weights normalised per output pixel), without its 22-bit rounding of the weights."""
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    R = np.zeros((out_size, in_size))
    for i in range(out_size):
        centre = (i + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), in_size)
        k = np.array([_bicubic((j - centre + 0.5) / fscale) for j in range(lo, hi)])
        R[i, lo:hi] = k / k.sum() if k.sum() != 0.0 else k
    return R


def box_radius(radius, passes=3):
    """The fractional box radius Pillow's GaussianBlur(radius) runs `passes` times per axis (BoxBlur.c, its float32 steps)."""
    f = np.float32
    radius = f(radius)
    sigma2 = f(radius * radius / f(passes))
    L = f(np.sqrt(12.0 * float(sigma2) + 1.0))
    l = f(np.floor((float(L) - 1.0) / 2.0))
    a = f(f(2 * l + 1) * f(l * f(l + 1) - f(3) * sigma2))
    a = f(a / f(f(6) * f(sigma2 - f(l + 1) * f(l + 1))))
    return float(f(l + a))


def box_matrix(n, fr):
    """(n, n) float64: one pass of the fractional box filter of radius `fr` with replicated edges: weight 1 / (2 fr + 1) on the
    2 int(fr) + 1 centre pixels, the rest shared by the two pixels beyond them."""
    r = int(fr)
    ww = 1.0 / (2.0 * fr + 1.0)
    fw = (1.0 - (2 * r + 1) * ww) / 2.0
    B = np.zeros((n, n))
    for i in range(n):
        for d in range(-r, r + 1):
            B[i, min(max(i + d, 0), n - 1)] += ww
        for j in (i - r - 1, i + r + 1):
            B[i, min(max(j, 0), n - 1)] += fw
    return B


def downblur_axis(in_size, out_size, blur_radius):
    """(out_size, in_size) float64: resample, then three box passes - one axis of the DownBlur degradation, un-rounded."""
    A = resample_matrix(in_size, out_size)
    if blur_radius > 0:
        fr = box_radius(blur_radius)
        if fr > 0:
            B = box_matrix(out_size, fr)
            A = B @ B @ B @ A
    return A


def _check_strength(strength):
    if isinstance(strength, bool) or not isinstance(strength, numbers.Real) or not math.isfinite(strength):
        raise ValueError(f"strength={strength!r} must be a finite number")
    return float(strength)


class SeparableOperator:
    """x (.., H, W) -> A_y x A_x^T (.., h, w), `A_y` (h, H) and `A_x` (w, W) float64."""

    def __init__(self, A_y, A_x):
        self.A_y, self.A_x = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (A_y, A_x))
        if self.A_y.ndim != 2 or self.A_x.ndim != 2 or min(self.A_y.shape + self.A_x.shape) < 1:
            raise ValueError(f"SeparableOperator needs two matrices, got shapes {self.A_y.shape} and {self.A_x.shape}")
        self._device, self._projectors = {}, {}

    from_matrices = classmethod(lambda cls, A_y, A_x: cls(A_y, A_x))

    @classmethod
    def downblur(cls, size_hw, magnification_factor, blur_radius, lr_hw=None):
        """The trainer's DownBlur degradation of an (H, W) image without its uint8 roundings and clip, with the reference's
        (W // m, H // m) output size: a non-square image comes out with its extents swapped (degradation.py).  `lr_hw` names
        the output size instead: the tiler's LR scene is (H // m, W // m)."""
        H, W = (int(s) for s in size_hw)
        m = int(magnification_factor)
        h, w = (W // m, H // m) if lr_hw is None else (int(s) for s in lr_hw)
        if m < 1 or h < 1 or w < 1:
            raise ValueError(f"downblur: {H}x{W} is too small for magnification {magnification_factor}")
        if isinstance(blur_radius, bool) or not isinstance(blur_radius, numbers.Real) or not blur_radius >= 0:
            raise ValueError(f"downblur: blur_radius={blur_radius!r} must be a number >= 0")
        return cls(downblur_axis(H, h, float(blur_radius)), downblur_axis(W, w, float(blur_radius)))

    @classmethod
    def box(cls, size_hw, m):
        """The mean over m x m blocks."""
        H, W = (int(s) for s in size_hw)
        m = int(m)
        if m < 1 or H < m or W < m or H % m or W % m:
            raise ValueError(f"box: {H}x{W} is no multiple of m={m}")
        return cls(np.kron(np.eye(H // m), np.full((1, m), 1.0 / m)), np.kron(np.eye(W // m), np.full((1, m), 1.0 / m)))

    @classmethod
    def mtf(cls, size_hw, m, g, lr_hw=None):
        """The sensor-MTF degradation of an (H, W) band (mtf.py): the Gaussian of gain `g` at the LR Nyquist
        frequency and decimation by m, replicated edges, as the dense matrices of its fp32 taps.  The LR size is (H // m, W // m),
        not swapped, unless `lr_hw` names it."""
        from . import mtf as _mtf
        m = _mtf._check_factor(m, "m")
        taps, left = _mtf.gaussian_taps(g, m)
        h, w = _mtf.lr_shape(size_hw, m, lr_hw)
        return cls(_mtf.dense_axis(size_hw[0], h, taps, left, m), _mtf.dense_axis(size_hw[1], w, taps, left, m))

    @property
    def hr_shape(self):
        return self.A_y.shape[1], self.A_x.shape[1]

    @property
    def lr_shape(self):
        return self.A_y.shape[0], self.A_x.shape[0]

    def apply(self, x):
        """A_y x A_x^T in float64 numpy (the host form; `degrade` is the device's)."""
        return self.A_y @ np.asarray(x, dtype=np.float64) @ self.A_x.T

    def matrices(self, device):
        """(A_y, A_x) as fp32 tensors on `device`, made once."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(a).to(torch.float32).to(device).contiguous() for a in (self.A_y, self.A_x))
        return self._device[device]

    def factors(self, damping=0.01):
        """The float64 pieces of the projector: per axis the thin SVD A = P diag(s) V^T, and the gain F_ij = s_i s_j / (s_i^2
        s_j^2 + damping^2) - 1 / (s_i s_j) at damping 0, where an axis whose condition number exceeds 1e6 raises.  Returns
        {"D_y", "D_x", "U_y", "U_x", "P_y", "P_x", "G", "s_y", "s_x"} with D = diag(s) V^T and U = V."""
        if isinstance(damping, bool) or not isinstance(damping, numbers.Real) or not (math.isfinite(damping) and damping >= 0):
            raise ValueError(f"damping={damping!r} must be a finite number >= 0")
        out = {}
        for ax, A in (("y", self.A_y), ("x", self.A_x)):
            P, s, Vt = np.linalg.svd(A, full_matrices=False)
            if damping == 0 and not (s[-1] > 0 and s[0] / s[-1] <= MAX_CONDITION):
                raise ValueError(f"the operator's {ax} axis has condition number {s[0] / s[-1] if s[-1] > 0 else math.inf:.3g} > "
                                 f"{MAX_CONDITION:g}: its exact pseudo-inverse amplifies rounding into the image; pass damping > 0")
            out["P_" + ax], out["s_" + ax], out["D_" + ax], out["U_" + ax] = P, s, s[:, None] * Vt, Vt.T.copy()
        ss = out["s_y"][:, None] * out["s_x"][None, :]
        out["G"] = 1.0 / ss if damping == 0 else ss / (ss * ss + float(damping) ** 2)
        return out

    def projector(self, damping=0.01, device="cuda"):
        """The `LRProjector` of this operator on `device`, made once per (damping, device)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (float(damping) if isinstance(damping, numbers.Real) else damping, device)
        if key not in self._projectors:
            self._projectors[key] = LRProjector(self, damping, device)
        return self._projectors[key]


MAX_OPERATORS = 16  # the band table of the kernels


class BandOperator:
    """One `SeparableOperator` per band: up to 16 operators of one shape and, for each of the C bands, the index of the one it
    uses.  It has the surface of a `SeparableOperator` on (.., C, H, W) images; its device tensors carry a leading n_ops axis
    and go to the *_bands entries with `band_op` (include/drs_hip.h)."""

    def __init__(self, operators, band_op):
        self.operators = list(operators)
        if not 1 <= len(self.operators) <= MAX_OPERATORS or not all(isinstance(o, SeparableOperator) for o in self.operators):
            raise ValueError(f"BandOperator needs 1 .. {MAX_OPERATORS} SeparableOperators")
        if any(o.hr_shape != self.operators[0].hr_shape or o.lr_shape != self.operators[0].lr_shape for o in self.operators):
            raise ValueError("BandOperator: the operators differ in shape")
        try:
            self.band_op = [int(b) for b in band_op]
        except (TypeError, ValueError):
            raise ValueError(f"BandOperator: band_op={band_op!r} must list one operator index per band") from None
        if not len(self.operators) <= len(self.band_op) <= MAX_OPERATORS:
            raise ValueError(f"BandOperator: {len(self.band_op)} bands for {len(self.operators)} operators (need n_ops <= bands <= "
                             f"{MAX_OPERATORS})")
        if min(self.band_op) < 0 or max(self.band_op) >= len(self.operators):
            raise ValueError(f"BandOperator: band_op={self.band_op} names an operator outside 0 .. {len(self.operators) - 1}")
        self._device, self._projectors = {}, {}

    @classmethod
    def mtf(cls, size_hw, m, gains, lr_hw=None):
        """One MTF operator per distinct gain of `gains` (C values); bands with equal gains share it (and its SVD)."""
        gains = [float(g) for g in gains]
        distinct = sorted(set(gains), key=gains.index)  # (the order of mtf.band_taps: the FIR's rows and these operators pair up)
        return cls([SeparableOperator.mtf(size_hw, m, g, lr_hw) for g in distinct], [distinct.index(g) for g in gains])

    @property
    def bands(self):
        return len(self.band_op)

    @property
    def hr_shape(self):
        return self.operators[0].hr_shape

    @property
    def lr_shape(self):
        return self.operators[0].lr_shape

    def apply(self, x):
        """Band c of x (.., C, H, W) through its own operator, in float64 numpy."""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim < 3 or x.shape[-3] != self.bands:
            raise ValueError(f"BandOperator.apply: x {x.shape} does not have {self.bands} bands")
        return np.stack([self.operators[o].apply(x[..., c, :, :]) for c, o in enumerate(self.band_op)], axis=-3)

    def matrices(self, device):
        """(A_y (n_ops, h, H), A_x (n_ops, w, W)) as fp32 tensors on `device`, made once."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = tuple(torch.from_numpy(np.stack([getattr(o, k) for o in self.operators])).to(torch.float32)
                                         .to(device).contiguous() for k in ("A_y", "A_x"))
        return self._device[device]

    def factors(self, damping=0.01):
        """`SeparableOperator.factors` of every operator, each key stacked along a leading n_ops axis."""
        per = [o.factors(damping) for o in self.operators]
        return {k: np.stack([f[k] for f in per]) for k in per[0]}

    projector = SeparableOperator.projector


class LRProjector:
    """The fp32 device tensors of the projection X' = X + strength U_y (G o (Yt - D_y X D_x^T)) U_x^T of `operator`, from its
    per-axis SVDs computed once in float64: D_y (h, H), D_x (w, W), U_y (H, h), U_x (W, w), G (h, w) and, for `prepare`,
    P_y^T (h, h) and P_x^T (w, w).  Of a `BandOperator`: each with a leading n_ops axis, and `band_op`, the operator of each band."""

    def __init__(self, operator, damping=0.01, device="cuda"):
        f = operator.factors(damping)
        self.operator, self.damping, self.device = operator, float(damping), torch.device(device)
        self.band_op = getattr(operator, "band_op", None)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(self.device).contiguous()
        self.D_y, self.D_x, self.U_y, self.U_x, self.G = (dev(f[k]) for k in ("D_y", "D_x", "U_y", "U_x", "G"))
        self.Pt_y, self.Pt_x = dev(np.swapaxes(f["P_y"], -1, -2)), dev(np.swapaxes(f["P_x"], -1, -2))

    @property
    def hr_shape(self):
        return self.operator.hr_shape

    @property
    def lr_shape(self):
        return self.operator.lr_shape

    def prepare(self, y):
        """Yt = P_y^T y P_x per plane of the observation y (B, C, h, w): made once per chain."""
        if tuple(y.shape[-2:]) != self.lr_shape:
            raise ValueError(f"the observation is {tuple(y.shape[-2:])}, the operator maps to {self.lr_shape}")
        if self.band_op is None:
            return hip_ops.sep_apply(y, self.Pt_y, self.Pt_x)
        if y.shape[1] != len(self.band_op):
            raise ValueError(f"the observation has {y.shape[1]} bands, the operator {len(self.band_op)}")
        return hip_ops.sep_apply(y, self.Pt_y, self.Pt_x, band_op=self.band_op)


class LRConsistency:
    """The request for LR-consistent sampling: `Diffusion.lr_consistency = LRConsistency(...)` (super-resolution only), the
    tiler's and `evaluate`'s `lr_consistency=`.  `blur_radius` None: the diffusion's own (`Diffusion.blur_radius`; "random" there
    needs a number here); `damping` the delta of the gain; `strength` 1 the full projection, 0 none; `operator` a
    `SeparableOperator` instead of the DownBlur one of the image size."""

    def __init__(self, blur_radius=None, damping=0.01, strength=1.0, operator=None):
        if blur_radius is not None and (isinstance(blur_radius, bool) or not isinstance(blur_radius, numbers.Real)
                                        or not blur_radius >= 0):
            raise ValueError(f"blur_radius={blur_radius!r} must be None or a number >= 0")
        if isinstance(damping, bool) or not isinstance(damping, numbers.Real) or not (math.isfinite(damping) and damping >= 0):
            raise ValueError(f"damping={damping!r} must be a finite number >= 0")
        if operator is not None and not isinstance(operator, (SeparableOperator, BandOperator)):
            raise ValueError("operator must be a SeparableOperator or a BandOperator")
        self.blur_radius = None if blur_radius is None else float(blur_radius)
        self.damping, self.strength, self.operator = float(damping), _check_strength(strength), operator

    def __repr__(self):
        return (f"LRConsistency(blur_radius={self.blur_radius}, damping={self.damping}, strength={self.strength}, "
                f"operator={self.operator})")

    def radius_for(self, diffusion):
        if self.blur_radius is not None:
            return self.blur_radius
        radius = getattr(diffusion, "blur_radius", 0.5)
        if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
            raise ValueError(f"lr_consistency: the diffusion's blur_radius is {radius!r}: pass LRConsistency(blur_radius=<number>)")
        return float(radius)

    def operator_for(self, diffusion, size_hw, lr_hw=None):
        """The operator of an (H, W) image: the explicit one, or the DownBlur of `diffusion` (ValueError for BSRGAN, which is
        neither linear nor fixed); `lr_hw` as `SeparableOperator.downblur`'s."""
        if self.operator is not None:
            if self.operator.hr_shape != tuple(size_hw):
                raise ValueError(f"lr_consistency: the operator takes {self.operator.hr_shape} images, the chain's are {tuple(size_hw)}")
            return self.operator
        what = self.check_for(diffusion)
        if isinstance(what, tuple):  # an MTF diffusion: its per-band gains
            return BandOperator.mtf(size_hw, diffusion.magnification_factor, what, lr_hw)
        return SeparableOperator.downblur(size_hw, diffusion.magnification_factor, what, lr_hw)

    def check_for(self, diffusion):
        """ValueError where `diffusion` gives the request no operator (BSRGAN, a "random" radius); the blur radius - for an MTF
        diffusion the tuple of its per-band Nyquist gains -, or None with an explicit operator.  Cheap: `sample_chain` asks
        before the engine is touched."""
        if self.operator is not None:
            return None
        kind = str(getattr(diffusion, "Degradation_type", "DownBlur")).lower()
        if kind == "mtf":
            if self.blur_radius is not None:
                raise ValueError("lr_consistency: blur_radius belongs to the DownBlur operator; an MTF diffusion's operator comes from "
                                 "its mtf_nyquist")
            gains = getattr(diffusion, "mtf_nyquist", None)
            if gains is None:
                raise ValueError("lr_consistency: the MTF diffusion has no mtf_nyquist")
            return tuple(float(g) for g in gains)
        if kind not in ("downblur", "downblurnoise"):
            raise ValueError(f"lr_consistency needs Degradation_type DownBlur, DownBlurNoise or MTF (got {kind!r}: no linear operator "
                             "describes it); pass LRConsistency(operator=...) to name one")
        return self.radius_for(diffusion)


# (H, W, m, radius | the tuple of MTF gains) -> the diffusion's own operator of the chains of that size (each keeps its projectors)
_OPERATORS = {}


def check_lr_consistency(request):
    if request is not None and not isinstance(request, LRConsistency):
        raise ValueError(f"lr_consistency={request!r} must be None or an LRConsistency")
    return request


def chain_projector(diffusion, request, size_hw, device):
    """The `LRProjector` of `request` for chains of (H, W) images of `diffusion`: made once per (H, W, m, radius, damping,
    device)."""
    if request.operator is not None:
        return request.operator_for(diffusion, size_hw).projector(request.damping, device)
    key = (int(size_hw[0]), int(size_hw[1]), int(diffusion.magnification_factor), request.check_for(diffusion))
    if key not in _OPERATORS:
        _OPERATORS[key] = request.operator_for(diffusion, size_hw)
    return _OPERATORS[key].projector(request.damping, device)


def _planes(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{what} must be a (B, C, H, W) tensor")
    return x


def degrade(x, op):
    """A_y x A_x^T per plane of x (B, C, H, W) fp32 on a ROCm device -> (B, C, h, w)."""
    _planes(x, "degrade: x")
    if tuple(x.shape[-2:]) != op.hr_shape:
        raise ValueError(f"degrade: x is {tuple(x.shape[-2:])}, the operator takes {op.hr_shape}")
    band_op = getattr(op, "band_op", None)
    if band_op is None:
        return hip_ops.sep_apply(x, *op.matrices(x.device))
    if x.shape[1] != len(band_op):
        raise ValueError(f"degrade: x has {x.shape[1]} bands, the operator {len(band_op)}")
    return hip_ops.sep_apply(x, *op.matrices(x.device), band_op=band_op)


def project(x0, y, projector, strength=1.0, out=None):
    """x0 (B, C, H, W) moved onto the images `projector`'s operator maps to y (B, C, h, w): X + strength U_y (G o (Yt - D_y X
    D_x^T)) U_x^T per plane; a new tensor, or `out` (which may be x0)."""
    _planes(x0, "project: x0"), _planes(y, "project: y")
    if tuple(x0.shape[-2:]) != projector.hr_shape or tuple(y.shape[:2]) != tuple(x0.shape[:2]):
        raise ValueError(f"project: x0 {tuple(x0.shape)} and y {tuple(y.shape)} do not fit the operator {projector.hr_shape} -> "
                         f"{projector.lr_shape}")
    strength = _check_strength(strength)
    return hip_ops.sep_project(x0, projector.prepare(y), projector, strength, out=out)


def lr_rmse(x, y, op):
    """(B,) fp32: per image, the root mean square of A x - y over bands and LR pixels."""
    d = degrade(x, op) - y
    return d.square().mean(dim=(1, 2, 3)).sqrt()
