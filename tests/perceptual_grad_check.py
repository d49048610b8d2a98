"""Float64 oracle of one superres training step with the MSE+Perceptual_noise loss (a plain module, imported by the tests).

grad_check.oracle_step fixes the loss to MSE; this is the same step (train-mode UNet forward of the CPU oracle, autograd
backward) with CombinedLoss(MSE, VGG, 0.3) of tests/vgg_oracle.py."""
import torch

import vgg_oracle as O
from grad_check import canonical, oracle_leaves


def oracle_step_combined(sd, vgg_sd, live, x, t, lr_img, noise, mag=2, dtype=torch.float64):
    """(loss, {live name: gradient or None}) of 0.3 * mse(pred, noise) + 0.7 * vgg(pred, noise)."""
    from oracle import unet_oracle as U
    live = set(live)
    leaves = oracle_leaves(sd, {canonical(n) for n in live}, dtype)
    pred = U.unet_forward(leaves, x.to(dtype), t, lr_img.to(dtype), mag, training=True, stats={})
    vsd = {k: v.to(dtype) for k, v in vgg_sd.items()}
    loss = O.combined_loss(vsd, pred, noise.to(dtype))
    loss.backward()
    grads = {n: (None if leaves[n].grad is None else leaves[n].grad.detach().clone()) for n in live}
    return loss.item(), grads
