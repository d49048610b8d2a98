"""Function-preserving channel rescalings of the superres UNet (test helper, not a conftest).

ReLU is positively homogeneous and BatchNorm / convolution are linear in their affine parameters, so the output channel c of
a layer can be multiplied by alpha[c] and the input column c of every layer reading it by 1 / alpha[c] without changing the
network's function in exact arithmetic.  A trained network drifts into exactly such scalings: the channels of one tensor then
span decades, and the kernels' per-block scales (csrc/conv_mfma_fl.hip) see them, while the whole-tensor metrics of the other
tests do not.  `rescale(sd, site, alpha)` applies one such edit; every BatchNorm alias of a registration gets the same edit
(synthetic.canonical_key).

Sites: the tensor whose channels are scaled, named like the oracle's taps (oracle/unet_oracle.py).
"""
import torch
import torch.nn.functional as F

from diffusionremotesensing_amd import synthetic

BLOCKS = ("conv_blocks.0", "conv_blocks.1", "conv_blocks.2", "bottle_neck")
SITES = tuple(f"{b}.h" for b in BLOCKS) + tuple(f"downs.{i}" for i in range(3)) + \
    tuple(f"attention_blocks.{i}" for i in range(3)) + tuple(f"ups.{i}.conv" for i in range(3)) + \
    tuple(f"gating_signals.{i}" for i in range(3)) + ("up_convs.2",)
# no ReLU between producer and consumer: alpha may be negative there
LINEAR_SITES = tuple(f"downs.{i}" for i in range(3)) + tuple(f"attention_blocks.{i}" for i in range(3)) + ("up_convs.2",)

FL_PACK_LIMIT = 60000.0  # largest folded weight the FL pack keeps (csrc/conv_mfma_fl.hip: fl_repack_kernel)


def _bn(prefix):
    return [(prefix + ".weight", "row"), (prefix + ".bias", "row")]


def _conv_row(prefix):
    return [(prefix + ".weight", "row"), (prefix + ".bias", "row")]


def edits(site):
    """(producer edits, consumer edits) of a site: lists of (canonical key, kind).  kind "row": dim 0 x alpha (weights, biases,
    BatchNorm affine parameters); ("col", c0): input columns c0 .. c0 + C - 1 of a convolution x 1 / alpha; "dim0": the input
    dimension of a ConvTranspose weight (Cin, Cout, kh, kw) x 1 / alpha."""
    if site.endswith(".h"):
        blk = site[:-2]
        prod = _bn(blk + ".batch_norm1") + _conv_row(blk + ".time_mlp.2")
        if blk == "conv_blocks.0":
            prod += _conv_row(blk + ".conv_upsampled_lr_img")
        return prod, [(blk + ".conv2.0.weight", ("col", 0))]
    kind, i = site.rsplit(".", 1) if site.count(".") == 1 else (site, None)
    if kind == "downs":
        nxt = BLOCKS[int(i) + 1]
        return _conv_row(site), [(nxt + ".conv1.0.weight", ("col", 0)), (nxt + ".shortcut_conv.0.weight", ("col", 0))]
    if kind == "attention_blocks":
        return _bn(site + ".result.1"), [(f"up_convs.{i}.weight", ("col", "att"))]
    if kind == "gating_signals":
        return _bn(site + ".batch_norm"), [(f"attention_blocks.{i}.w_g.0.weight", ("col", 0))]
    if kind == "up_convs":
        return _conv_row(site), [("output.weight", ("col", 0))]
    if site.startswith("ups.") and site.endswith(".conv"):
        ups = site[: -len(".conv")]
        return _bn(ups + ".batch_norm"), [(ups + ".transform.weight", "dim0")]
    raise KeyError(site)


def _keys(sd, canon):
    keys = [k for k in sd if synthetic.canonical_key(k) == canon]
    if not keys:
        raise KeyError(canon)
    return keys


def _scale(t, kind, alpha, sd, key):
    C = alpha.numel()
    a = alpha.to(t.dtype)
    if kind == "row":
        return t * a.view((-1,) + (1,) * (t.dim() - 1))
    if kind == "dim0":
        return t / a.view(-1, 1, 1, 1)
    c0 = kind[1]
    if c0 == "att":  # up_convs.i reads cat([ups.i, att]): the att-half starts after Cout(ups.i)
        i = key.split(".")[1]
        c0 = sd[f"ups.{i}.transform.weight"].shape[1]
    out = t.clone()
    out[:, c0:c0 + C] = out[:, c0:c0 + C] / a.view(1, -1, 1, 1)
    return out


def channels(sd, site):
    prod, _ = edits(site)
    return sd[_keys(sd, prod[0][0])[0]].shape[0]


def rescale(sd, site, alpha):
    """A new state_dict (the input is not modified) with the tensor `site` scaled per channel by `alpha` (shape (C,)) and its
    readers compensated: the same function in exact arithmetic."""
    alpha = torch.as_tensor(alpha, dtype=torch.float64).flatten()
    C = channels(sd, site)
    if alpha.numel() != C:
        raise ValueError(f"{site}: {C} channels, alpha has {alpha.numel()}")
    if bool((alpha == 0).any()) or not bool(torch.isfinite(alpha).all()):
        raise ValueError(f"{site}: alpha must be finite and non-zero")
    if site not in LINEAR_SITES and bool((alpha < 0).any()):
        raise ValueError(f"{site}: a ReLU sits between producer and consumer, alpha must be positive")
    out = dict(sd)
    prod, cons = edits(site)
    for canon, kind in prod + cons:
        for key in _keys(sd, canon):
            out[key] = _scale(out[key], kind, alpha, sd, key)
    return out


# ---- folded weights (what the pack of the eval plan sees) ----------------------------------------------------------------------
def bn_fold(sd, bn):
    """gamma / sqrt(running_var + eps) of an eval-mode BatchNorm (BN_EPS of the oracle)."""
    return sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)


def producer_rows(sd, site):
    """|folded producer weight| maxima per channel of `site` (the convolution that writes it, BatchNorm folded in), or None
    where the producer is no convolution of the eval plan's own (the gating / attention / time-MLP compositions)."""
    if site.endswith(".h"):
        blk = site[:-2]
        w = sd[blk + ".conv1.0.weight"].double() * bn_fold(sd, blk + ".batch_norm1").view(-1, 1, 1, 1)
    elif site.startswith("downs.") or site == "up_convs.2":
        w = sd[site + ".weight"].double()
    elif site.startswith("ups."):
        ups = site[: -len(".conv")]
        w = sd[ups + ".conv.weight"].double() * bn_fold(sd, ups + ".batch_norm").view(-1, 1, 1, 1)
    elif site.startswith("gating_signals."):
        w = sd[site + ".conv.weight"].double() * bn_fold(sd, site + ".batch_norm").view(-1, 1, 1, 1)
    elif site.startswith("attention_blocks."):
        w = sd[site + ".result.0.weight"].double() * bn_fold(sd, site + ".result.1").view(-1, 1, 1, 1)
    else:
        raise KeyError(site)
    return w.abs().flatten(1).amax(1)


def consumer_cols(sd, site):
    """|folded consumer weight| maxima per channel of `site` over every reader (BatchNorm behind the reader folded in)."""
    _, cons = edits(site)
    best = None
    for canon, kind in cons:
        w = sd[canon].double()
        if kind == "dim0":
            m = w.abs().flatten(1).amax(1)
        else:
            layer = canon[: -len(".weight")]
            bn = {".conv1.0": ".batch_norm1", ".conv2.0": ".batch_norm2", ".shortcut_conv.0": ".shortcut_batch_norm"}
            for suf, b in bn.items():
                if layer.endswith(suf):
                    w = w * bn_fold(sd, layer[: -len(suf)] + b).view(-1, 1, 1, 1)
            c0 = kind[1]
            if c0 == "att":
                c0 = sd[f"ups.{canon.split('.')[1]}.transform.weight"].shape[1]
            C = channels(sd, site)
            m = w[:, c0:c0 + C].abs().transpose(0, 1).flatten(1).amax(1)
        best = m if best is None else torch.maximum(best, m)
    return best


# ---- metrics ---------------------------------------------------------------------------------------------------------------
def per_channel_rel_l2(got, want, floor=None):
    """rel-L2 of every channel of an NCHW tensor against its OWN norm (over batch and pixels); the worst channel and its index.
    A channel that is 1e-3 of the tensor's scale is invisible to a whole-tensor metric and fully visible here.  `floor` (per
    channel, optional): the smallest norm a channel is measured against - for channels that are near zero on the ORIGINAL
    weights (a ReLU output whose terms cancel), where rel-L2 measures the cancellation rather than the arithmetic."""
    g = torch.as_tensor(got).double().transpose(0, 1).flatten(1)
    w = torch.as_tensor(want).double().transpose(0, 1).flatten(1)
    num = (g - w).norm(dim=1)
    den = w.norm(dim=1)
    if floor is not None:
        den = torch.maximum(den, torch.as_tensor(floor, dtype=torch.float64))
    rel = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))
    worst = int(rel.argmax())
    return float(rel[worst]), worst


def extra_taps(sd, taps, t):
    """Quantities the HIP plan keeps under names the oracle does not tap, recomputed in the oracle's dtype from its taps:
    `cond` (conditioning convolution), `conv_blocks.0.skip`, `ups.i.in` (x + relu(time_mlp(t)): the decoder stage inputs that
    DRS_XT_ONLY plans store instead of x), `attention_blocks.i.g1` / `.relu` and `cat.i`."""
    from oracle import unet_oracle as U
    temb = U.pos_encoding(t.unsqueeze(-1).float(), U.TIME_EMB_DIM).to(taps["x0"].dtype)
    out = {"cond": U._conv(sd, "conv_upsampled_lr_img", taps["upsampled_lr_img"], padding=1),
           "conv_blocks.0.skip": U._conv(sd, "conv_blocks.0.conv_upsampled_lr_img", taps["x0"], padding=1)}
    residual = ("conv_blocks.2", "conv_blocks.1", "conv_blocks.0")
    for i in range(3):
        x = taps["bottle_neck"] if i == 0 else taps[f"up_convs.{i - 1}"]
        out[f"ups.{i}.in"] = x + U._time_mlp(sd, f"ups.{i}.time_mlp", temb)
        g1 = U._conv(sd, f"attention_blocks.{i}.w_g.0", taps[f"gating_signals.{i}"])
        x1 = U._conv(sd, f"attention_blocks.{i}.w_x.0", taps[residual[i]], stride=2)
        out[f"attention_blocks.{i}.g1"] = g1
        out[f"attention_blocks.{i}.relu"] = F.relu(g1 + x1)
        out[f"cat.{i}"] = torch.cat([taps[f"ups.{i}"], taps[f"attention_blocks.{i}"]], dim=1)
    return out
