"""Fine-tuning a snapshot (`Diffusion.train(..., freeze_bn=, freeze=, init_from=)`, `--freeze_bn --freeze --init_from`;
DESIGN.md section 25): the host pieces around the frozen-BatchNorm train plan (engine.py, csrc/bn_train.hip).

- `freeze_parameters`: state_dict-key prefixes -> `requires_grad_(False)`; the engine then hands drs_unet_backward a NULL slot
  for each of them and the optimizers skip what has no gradient.
- `load_init_weights`: the MODEL_STATE of another run's snapshot as the start of a new run (epoch 0, no optimizer state).
"""
import torch


def frozen_names(net, prefixes):
    """Names of the parameters whose state_dict key starts with one of `prefixes`, in `named_parameters()` order.
    ValueError for a prefix that matches no parameter (a typo would otherwise train everything, silently)."""
    prefixes = tuple(prefixes)
    names = [n for n, _ in net.named_parameters()]
    for pre in prefixes:
        if not isinstance(pre, str) or not pre or not any(n.startswith(pre) for n in names):
            raise ValueError(f"freeze: prefix {pre!r} matches no parameter of the model (state_dict keys start with "
                             f"{sorted({n.split('.')[0] + '.' for n in names})})")
    return [n for n in names if n.startswith(prefixes)] if prefixes else []


def freeze_parameters(net, prefixes):
    """`requires_grad_(False)` on every parameter `frozen_names` finds; returns (frozen, trained) counts of parameter
    tensors and (frozen, trained) counts of their elements.  ValueError when nothing is left to train."""
    frozen = set(frozen_names(net, prefixes))
    for n, p in net.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    params = list(net.parameters())
    off = [p for p in params if not p.requires_grad]
    on = [p for p in params if p.requires_grad]
    if not on:
        raise ValueError(f"freeze: {tuple(prefixes)} leaves no parameter to train")
    return (len(off), len(on)), (sum(p.numel() for p in off), sum(p.numel() for p in on))


def load_init_weights(net, path, prediction="eps", map_location="cpu"):
    """Loads `MODEL_STATE` of the snapshot `path` into `net` (EPOCHS_RUN is ignored: the new run starts at epoch 0).
    ValueError when the snapshot's network predicts something else than `prediction` (a file without the key: eps), when a
    key is missing or unknown, or - naming the key - when a tensor has another shape."""
    snapshot = torch.load(path, map_location=map_location)
    saved = snapshot.get("PREDICTION", "eps")
    if saved != prediction:
        raise ValueError(f"{path} holds a network that predicts {saved!r}, this run was built with prediction={prediction!r} "
                         f"(--prediction {saved})")
    state = {k.replace("module.", ""): v for k, v in snapshot["MODEL_STATE"].items()}
    own = net.state_dict()
    for k, v in state.items():
        if k in own and tuple(own[k].shape) != tuple(v.shape):
            raise ValueError(f"init_from {path}: {k} has shape {tuple(v.shape)}, the model's is {tuple(own[k].shape)} "
                             "(another band count or class count?)")
    if set(state) != set(own):
        raise ValueError(f"init_from {path}: keys differ from the model's: {sorted(set(state) ^ set(own))[:6]}")
    net.load_state_dict(state)
    return net
