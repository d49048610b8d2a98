"""Seeded, version-independent synthetic weights and inputs.

The reference ships no pretrained weights (`/root/reference/.MISSING_LARGE_BLOBS`),
so parity is checked on weights produced by a counter-based generator that is
keyed by the state_dict key name.  The generator is plain integer arithmetic
(splitmix64 -> Box-Muller) on numpy uint64, so the golden-vector script in this
container, the tests and the bench on the GPU box all regenerate bit-identical
tensors without shipping 17.5 MB of weights.

BatchNorm statistics and affine parameters are randomised on purpose: a
fresh-init BatchNorm is the identity in eval mode and would test nothing
(SURVEY.md section 8(c)).
"""
import zlib

import numpy as np
import torch

_MASK = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & _MASK
    z = x
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _MASK
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _MASK
    return z ^ (z >> np.uint64(31))


def _key_seed(key, seed):
    return np.uint64(zlib.crc32(key.encode()) | (int(seed) & 0xFFFFFFFF) << 32)


def uniform01(key, n, seed=0):
    """n float64 uniforms in (0,1), a pure function of (key, seed, index)."""
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + _key_seed(key, seed)
        bits = _splitmix64(_splitmix64(ctr))
    return ((bits >> np.uint64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def normal(key, n, seed=0):
    u1 = uniform01(key + "#a", n, seed)
    u2 = uniform01(key + "#b", n, seed)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def tensor_normal(key, shape, seed=0, std=1.0, mean=0.0):
    n = int(np.prod(shape)) if len(shape) else 1
    a = (normal(key, n, seed) * std + mean).astype(np.float32)
    return torch.from_numpy(a.reshape(shape))


def tensor_uniform(key, shape, seed=0, lo=0.0, hi=1.0):
    n = int(np.prod(shape)) if len(shape) else 1
    a = (uniform01(key, n, seed) * (hi - lo) + lo).astype(np.float32)
    return torch.from_numpy(a.reshape(shape))


def tensor_randint(key, shape, lo, hi, seed=0):
    """int64 in [lo, hi)."""
    n = int(np.prod(shape)) if len(shape) else 1
    a = np.floor(uniform01(key, n, seed) * (hi - lo)).astype(np.int64) + lo
    return torch.from_numpy(a.reshape(shape))


def block_mask(name, n, size, fraction, block, seed=0):
    """(n, 1, size, size) uint8 "cloud" masks, 1 = known: every image hides a union of block x block squares at seeded
    positions, added one by one until at least `fraction` of its pixels are hidden - so the hidden share lies in
    [fraction, fraction + block^2 / size^2).  A pure function of its arguments, like the other generators."""
    if not 0.0 <= fraction <= 1.0:
        raise ValueError(f"block_mask: fraction={fraction} outside [0, 1]")
    if not 1 <= block <= size:
        raise ValueError(f"block_mask: block={block} outside [1, size = {size}]")
    target, span = fraction * size * size, size - block + 1
    known = np.ones((n, 1, size, size), dtype=np.uint8)
    for i in range(n):
        hidden, chunk = 0, 0
        while hidden < target:
            pos = np.floor(uniform01(f"{name}.{i}.{chunk}", 512, seed) * span).astype(np.int64)
            for y, x in zip(pos[0::2], pos[1::2]):
                if hidden >= target:
                    break
                known[i, 0, y:y + block, x:x + block] = 0
                hidden = known[i, 0].size - int(known[i, 0].sum())
            chunk += 1
    return torch.from_numpy(known)


def seeded_state_dict(template, seed=0):
    """Fill every entry of `template` (a state_dict: key -> tensor, only shapes and
    dtypes are used) with seeded values.  Aliased BatchNorm registrations
    (`...batch_norm1.*` and `...conv1.1.*`, UNet_model_superres.py:118-141 in the
    reference) receive identical values because both names are canonicalised to
    the same generator key.
    """
    out = {}
    for key, ref in template.items():
        ckey = canonical_key(key)
        shape = tuple(ref.shape)
        leaf = key.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[key] = torch.tensor(7, dtype=torch.int64)
        elif leaf == "running_mean":
            out[key] = tensor_normal(ckey, shape, seed, std=0.2)
        elif leaf == "running_var":
            out[key] = tensor_uniform(ckey, shape, seed, 0.5, 1.5)
        elif len(shape) == 1 and _is_bn_key(key):
            if leaf == "weight":
                out[key] = tensor_uniform(ckey, shape, seed, 0.6, 1.4)
            else:
                out[key] = tensor_normal(ckey, shape, seed, std=0.1)
        elif key == "label_emb.weight":
            out[key] = tensor_normal(ckey, shape, seed, std=1.0)  # nn.Embedding's own N(0, 1) scale
        elif leaf == "bias":
            out[key] = tensor_normal(ckey, shape, seed, std=0.05)
        else:
            fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            if "transform" in key:
                # ConvTranspose2d weight is (Cin, Cout, kh, kw); 9 taps over 4 output phases
                fan_in = shape[0] * 9 // 4
            # gain chosen so that eval-mode activations stay O(1) through the residual/concat structure
            # (a trained network's BatchNorm statistics would do that; random ones do not)
            gain = 0.65 if (len(shape) == 4 and not key.startswith(("LR_encoder", "SAR_encoder"))) else 1.0
            out[key] = tensor_normal(ckey, shape, seed, std=gain * float(np.sqrt(2.0 / max(fan_in, 1))))
    return out


_BN_ALIASES = (
    (".conv1.1.", ".batch_norm1."),
    (".conv2.1.", ".batch_norm2."),
    (".shortcut_conv.1.", ".shortcut_batch_norm."),
)


def canonical_key(key):
    for alias, canon in _BN_ALIASES:
        if alias in key:
            return key.replace(alias, canon)
    return key


def _is_bn_key(key):
    k = canonical_key(key)
    return ("batch_norm" in k) or (".result.1." in k)


# BatchNorm registration (canonical prefix) -> the convolution in front of it
_BN_CONV = (
    (".batch_norm1", ".conv1.0"), (".batch_norm2", ".conv2.0"), (".shortcut_batch_norm", ".shortcut_conv.0"),
    (".result.1", ".result.0"),
)


def _conv_of_bn(bn_prefix):
    for bn, conv in _BN_CONV:
        if bn_prefix.endswith(bn):
            return bn_prefix[: -len(bn)] + conv
    if bn_prefix.endswith(".batch_norm"):  # gating_signals.i / ups.i
        return bn_prefix[: -len(".batch_norm")] + ".conv"
    raise KeyError(bn_prefix)


def trained_like_state_dict(template, calibrate, seed=0, bare_gain=1.0, tweak=None):
    """Seeded weights with the dynamic range a TRAINED snapshot folds into the kernels' operands, which freshly seeded ones
    (running_var 0.5 .. 1.5, gamma 0.6 .. 1.4) never show:
      * every convolution in front of a BatchNorm has its output channels scaled by 10^-1.5 .. 1 (log-uniform), so the
        statistics the BatchNorm holds span three decades (running_var down to ~1e-3 and below) and the folded weights
        gamma / sqrt(var) * w carry the inverse of it;
      * gamma 0.1 .. 10 (log-uniform), beta ~ N(0, 0.3);
      * the bare convolutions (`downs.*`, `up_convs.*`: no BatchNorm behind them) scaled by `bare_gain`: their outputs - inputs
        of the next wide 3x3 layers - grow by that factor;
      * `tweak(sd)`, if given, edits the weights further (in place) before the calibration;
      * running_mean / running_var are then CALIBRATED: `calibrate(sd)` runs a train-mode forward of the oracle on a batch and
        returns {bn_prefix: (batch_mean, batch_var)}, as the running averages of a converged training would be.
    All BatchNorm aliases of a registration receive the same values."""
    sd = seeded_state_dict(template, seed)
    groups = {}
    for key in sd:
        if _is_bn_key(key):
            groups.setdefault(canonical_key(key).rsplit(".", 1)[0], []).append(key)
    for bn, keys in groups.items():
        C = sd[bn + ".weight"].shape[0]
        s = 10.0 ** tensor_uniform(bn + ".tl.s", (C,), seed, -1.5, 0.0)
        gamma = 10.0 ** tensor_uniform(bn + ".tl.g", (C,), seed, -1.0, 1.0)
        beta = tensor_normal(bn + ".tl.b", (C,), seed, std=0.3)
        conv = _conv_of_bn(bn)
        sd[conv + ".weight"] = sd[conv + ".weight"] * s.view(-1, 1, 1, 1)
        sd[conv + ".bias"] = sd[conv + ".bias"] * s
        for key in keys:
            leaf = key.rsplit(".", 1)[-1]
            if leaf == "weight":
                sd[key] = gamma.clone()
            elif leaf == "bias":
                sd[key] = beta.clone()
    if bare_gain != 1.0:
        for key in sd:
            if key.startswith(("downs.", "up_convs.")):
                sd[key] = sd[key] * bare_gain
    if tweak is not None:
        tweak(sd)
    stats = calibrate(sd)
    for bn, keys in groups.items():
        mean, var = stats[bn]
        for key in keys:
            leaf = key.rsplit(".", 1)[-1]
            if leaf == "running_mean":
                sd[key] = mean.clone()
            elif leaf == "running_var":
                sd[key] = var.clone()
    return sd
