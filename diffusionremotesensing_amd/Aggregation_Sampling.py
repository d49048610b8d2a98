"""Drop-in `split_aggregation_sampling` (reference Aggregation_Sampling.py:9-138): super-resolve an image larger than
the UNet's training size tile by tile and blend the tiles with Gaussian weights.

Kept from the reference: constructor signature and attributes, `patchifier` (tile coordinates, including the
clamped-last-tile rule and the de-duplication), `gaussian_weights` (including its asymmetric midpoints: (W-1)/2 along x,
H/2 along y, :133-137), the accumulation order and the final normalise + clamp.

MI355X-first differences:
  * all tiles run through ONE `Diffusion.sample` call as a batch with one LR tile per sample (the reference runs
    len(tiles) sequential n=1 chains, 1499 batch-1 forwards each); under torch.distributed the tiles are sharded over the
    ranks (independent chains, no collective in the loop) and gathered once;
  * blend + normalise + clamp is one gather kernel (`drs_aggregate_tiles`) instead of two full-size accumulators and
    4 element-wise passes per tile.
Noise: the reference draws x_T and every z_i tile after tile from the global CPU generator; a batched run cannot
reproduce that stream order, so by default the n tiles draw one (n,C,S,S) tensor per step.  `noise_source(tile, i,
shape)` lets a caller (the parity tests) supply the reference's per-tile draws.

Not in the reference: `aggregation="per_step"` (`sample_scene`), the aggregation sampling of StableSR the class is named
after.  ONE state of scene size is denoised and the tiles' noise predictions are blended at every reverse step, so that
neighbouring tiles denoise the same pixels of an overlap from the same state instead of hallucinating unrelated detail
that the final blend can only average.  Opt-in: the default, "final", is the reference's behaviour bit for bit.
"""
from math import exp, pi, sqrt

import numpy as np
import torch

from . import dist as drs_dist
from . import hip_ops


# tiles per sampling chain (per rank): bounds the plan workspace (~0.1 GB per 256x256 tile) independently of the scene size
TILE_BATCH = 16


class split_aggregation_sampling:
    def __init__(self, img_lr, patch_size, stride, magnification_factor, diffusion_model, device):
        assert stride <= patch_size
        self.img_lr = img_lr
        self.patch_size = patch_size
        self.stride = stride
        self.magnification_factor = magnification_factor
        self.diffusion_model = diffusion_model
        self.device = device
        self.model = diffusion_model.model
        batch_size, channels, height, width = img_lr.shape
        self.patches_lr, self.patches_sr_infos = self.patchifier(img_lr, patch_size, stride, magnification_factor)
        self.weight = self.gaussian_weights(patch_size * magnification_factor, patch_size * magnification_factor,
                                            batch_size)

    def patchifier(self, img_to_split, patch_size, stride=None, magnification_factor=1):
        """Reference :24-68: tiles on a `stride` grid, the last one of a row / column clamped to the border,
        duplicates dropped; infos are (y0, y1, x0, x1) in super-resolved coordinates."""
        if stride is None:
            stride = patch_size
        batch_size, channels, height, width = img_to_split.shape
        patches_lr, patches_sr_infos = [], []
        m = magnification_factor
        for y in range(0, height + 1, stride):
            for x in range(0, width + 1, stride):
                y_start, y_end = (height - patch_size, height) if y + patch_size > height else (y, y + patch_size)
                x_start, x_end = (width - patch_size, width) if x + patch_size > width else (x, x + patch_size)
                info = (y_start * m, y_end * m, x_start * m, x_end * m)
                if info not in patches_sr_infos:
                    patches_lr.append(img_to_split[:, :, y_start:y_end, x_start:x_end])
                    patches_sr_infos.append(info)
        return patches_lr, patches_sr_infos

    def gaussian_weights(self, tile_width, tile_height, nbatches):
        """Reference :118-138 (float64 Python arithmetic, then float32; tiled to (nbatches, 3, H, W))."""
        var = 0.01
        midpoint = (tile_width - 1) / 2
        x_probs = [exp(-(x - midpoint) * (x - midpoint) / (tile_width * tile_width) / (2 * var)) / sqrt(2 * pi * var)
                   for x in range(tile_width)]
        midpoint = tile_height / 2
        y_probs = [exp(-(y - midpoint) * (y - midpoint) / (tile_height * tile_height) / (2 * var)) / sqrt(2 * pi * var)
                   for y in range(tile_height)]
        weights = torch.tensor(np.outer(y_probs, x_probs)).to(torch.float32).to(self.device)
        return torch.tile(weights, (nbatches, 3, 1, 1))

    def sample_tiles(self, noise_source=None, sampling_steps=None, eta=0.0):
        """Super-resolve every tile: (n_tiles, C, S, S) on this rank's device.  One batched chain (sharded over the
        ranks of an initialised process group); `sampling_steps` / `eta` select a DDIM chain (`Diffusion.sample`)."""
        d = self.diffusion_model
        lr = torch.cat([p[:1] for p in self.patches_lr], dim=0).to(self.device).contiguous()  # (n, C, ps, ps)
        n = lr.shape[0]
        lo, hi = drs_dist.shard_range(n) if drs_dist.world_size() > 1 else (0, n)
        src = None
        if noise_source is not None:
            def src(i, shape, lo=lo):  # stack the per-tile draws of this rank's tiles
                return torch.cat([noise_source(lo + k, i, (1,) + tuple(shape[1:])) for k in range(shape[0])], dim=0)
        # fixed-size chunks of this rank's tiles: one chain per chunk, ONE plan / workspace whatever the scene size (a
        # 2048 x 2048 scene at stride 32 has ~4000 tiles: as a single batch its workspace would not fit any device).
        # The last chunk is padded with repeats of its last tile so that it runs on the same plan.
        chunk = max(1, int(getattr(self, "tile_batch", 0) or TILE_BATCH))
        # the DDIM arguments are passed only when set: the default call is the reference's, whatever sampler `d` is
        ddim = {"sampling_steps": sampling_steps, "eta": eta} if sampling_steps is not None or eta != 0.0 else {}
        outs = []
        for c0 in range(lo, hi, chunk):
            c1 = min(c0 + chunk, hi)
            take = c1 - c0
            size = take if (hi - lo) <= chunk else chunk  # a scene smaller than one chunk runs at its own size
            lr_c = lr[c0:c1]
            if size > take:
                lr_c = torch.cat([lr_c, lr_c[-1:].expand(size - take, -1, -1, -1)], dim=0).contiguous()
            csrc = None
            if src is not None:
                def csrc(i, shape, c0=c0, take=take):
                    real = src(i, (take,) + tuple(shape[1:]), lo=c0)
                    if shape[0] > take:
                        real = torch.cat([real, real[-1:].expand(shape[0] - take, -1, -1, -1)], dim=0)
                    return real
            out_c = d.sample(size, self.model, lr_c, input_channels=lr.shape[1], generate_video=False, noise_source=csrc,
                             **ddim)
            outs.append(out_c[:take])
        mine = torch.cat(outs, dim=0) if outs else lr.new_zeros((0, lr.shape[1], d.image_size, d.image_size))
        if drs_dist.world_size() > 1:
            mine = drs_dist.gather_shards(mine, n)
        return mine

    def sample_scene(self, noise_source=None, sampling_steps=None, eta=0.0):
        """The joint reverse chain of the whole scene: the un-clamped (C, H*m, W*m) state after the last step.

        Protocol.  The state X has scene size.  x_T is `noise_source(T, (1, C, Hs, Ws))` or torch.randn on the CPU
        generator, the noise of step i `noise_source(i, (1, C, Hs, Ws))` or torch.randn_like(X), under the rules of
        `Diffusion._sample_chain` (none at i == 1; a DDIM chain draws only when sigma > 0, so eta = 0 draws x_T and nothing
        else).  Note the signature: a scene-level `noise_source(i, shape)`, not the final mode's per-tile one.
        One step cuts X into the tiles (`gather_tiles`), runs the UNet on them in chunks of `tile_batch` (the last chunk
        padded with repeats of its last tile, whose eps is never read), each forward writing its slice of ONE eps buffer,
        and takes the step with one `blend_step_`: per scene element the Gaussian-weighted mean of the covering tiles' eps,
        summed in tile index order, then the ancestral / DDIM / DPM-Solver++(2M) update of the per-tile samplers (the last with
        `sampling_steps=sampling_plan(S, solver="dpmpp_2m")`; its history is one more tensor of scene size, owned by the chain).
        Memory: the eps buffer holds every tile of a step, ceil(n / chunk) * chunk x (C, S, S) fp32: 0.79 MB per 256x256x3
        tile (38 MB for the 48 tiles of a 896x1152 scene, 3.1 GB for the ~4000 tiles of a 2048x2048 scene at stride 32),
        next to one chunk of gathered tiles and the plan's workspace.
        Conditioning: with one chunk the LR branch is computed on the first step and reused; with several chunks the
        plan's conditioning belongs to whichever chunk ran last, so every forward recomputes it.
        The loop is `run_reverse_chain`: the fault-word reads and the range-fault roll-back act on the scene state."""
        from .sampling import check_sampling_args
        d = self.diffusion_model
        check_sampling_args(d.noise_steps, sampling_steps, eta)
        if drs_dist.world_size() > 1:
            raise NotImplementedError(
                "aggregation='per_step' runs on one rank: the joint chain would need an all-gather of eps and a shared "
                "noise draw per step; use aggregation='final', which shards its independent tile chains over the ranks")
        batch_size, channels, height, width = self.img_lr.shape
        m = self.magnification_factor
        S = self.patch_size * m
        Hs, Ws = height * m, width * m
        lr = torch.cat([p[:1] for p in self.patches_lr], dim=0).to(self.device).contiguous()  # (n, C, ps, ps)
        n = lr.shape[0]
        chunk = max(1, int(getattr(self, "tile_batch", 0) or TILE_BATCH))
        size = n if n <= chunk else chunk  # a scene smaller than one chunk runs at its own size, like sample_tiles
        starts = list(range(0, n, size))
        lr_chunks = []
        for c0 in starts:
            lr_c = lr[c0:c0 + size]
            if lr_c.shape[0] < size:
                lr_c = torch.cat([lr_c, lr_c[-1:].expand(size - lr_c.shape[0], -1, -1, -1)], dim=0)
            lr_chunks.append(lr_c.contiguous())
        dev = lr.device
        origins = hip_ops.tile_origins([(info[0], info[2]) for info in self.patches_sr_infos], S, Hs, Ws, dev)
        weight = self.weight[0, 0].contiguous()
        eps_buf = torch.empty((len(starts) * size, channels, S, S), dtype=torch.float32, device=dev)
        x_tiles = torch.empty((size, channels, S, S), dtype=torch.float32, device=dev)
        uncovered = torch.zeros(1, dtype=torch.int32, device=dev)
        single = len(starts) == 1

        def predict(engine, x, t, first):
            for j, c0 in enumerate(starts):
                hip_ops.gather_tiles(x[0], origins, S, out=x_tiles, first=c0, count=size)
                engine.forward(x_tiles, t, lr_chunks[j], m, reuse_cond=single and not first,
                               check_weights=first and j == 0, out=eps_buf[c0:c0 + size])
            return eps_buf

        def update(x, eps, noise, i, i_prev, hist=None, t_q=-1):
            hip_ops.blend_step_(x[0], eps, origins, weight, noise[0] if noise is not None else None, i,
                                alpha_hat=d.alpha_hat, alpha=d.alpha, beta=d.beta, t_prev=i_prev, eta=eta,
                                uncovered=uncovered, hist=hist[0] if hist is not None else None, t_q=t_q)

        x = d._sample_chain(self.model, (1, channels, Hs, Ws), predict, table_rows=size, generate_video=False,
                            noise_source=noise_source, sampling_steps=sampling_steps, eta=eta, update=update)
        if int(uncovered.item()) != 0:
            raise AssertionError("aggregation: some scene pixels are covered by no tile (pixel_count == 0)")
        return x[0]

    def aggregation_sampling(self, noise_source=None, sampling_steps=None, eta=0.0, aggregation="final", color_fix=None,
                             color_fix_levels=5):
        """Reference :76-116 (`sampling_steps` / `eta`: every tile runs a DDIM chain).  `aggregation`: "final" (the
        reference: independent tile chains, blended once; `noise_source(tile, i, shape)`) or "per_step" (`sample_scene`:
        one joint chain, blended at every step; `noise_source(i, scene_shape)`), clamped to [0, 1].
        `color_fix`: None (the default: nothing changes), "wavelet" (with `color_fix_levels`) or "adain" - the finished, clamped
        scene is corrected once as a whole, never per tile, against the bicubic up-sampling of img_lr's first image
        (`colorfix.color_fix`) and clamped to [0, 1] again."""
        if aggregation not in ("final", "per_step"):
            raise ValueError(f"aggregation={aggregation!r} must be 'final' or 'per_step'")
        fix = self._color_fix(color_fix, color_fix_levels)
        batch_size, channels, height, width = self.img_lr.shape
        m = self.magnification_factor
        if aggregation == "per_step":
            out = fix(torch.clamp(self.sample_scene(noise_source, sampling_steps=sampling_steps, eta=eta), 0, 1))
            return out.unsqueeze(0).expand(batch_size, -1, -1, -1).contiguous()
        tiles = self.sample_tiles(noise_source, sampling_steps=sampling_steps, eta=eta)
        origins = [(info[0], info[2]) for info in self.patches_sr_infos]
        out = fix(hip_ops.aggregate_tiles(tiles, origins, self.weight[0, 0].contiguous(), height * m, width * m))
        # the reference broadcasts the single chain of each tile over the batch dimension of img_lr
        return out.unsqueeze(0).expand(batch_size, -1, -1, -1).contiguous()

    def _color_fix(self, method, levels):
        """f(clamped scene (C, Hs, Ws)) -> the scene `aggregation_sampling` returns: the identity without a method (checked
        here, before anything is sampled)."""
        if method is None:
            return lambda scene: scene
        from .colorfix import color_fix, fix_levels
        levels = fix_levels(method, levels)

        def fix(scene):
            lr = self.img_lr[:1].to(scene.device, torch.float32).contiguous()
            fixed = color_fix(scene.unsqueeze(0), lr, magnification_factor=self.magnification_factor, method=method,
                              levels=levels)
            return torch.clamp(fixed[0], 0, 1)
        return fix


def launch(args):
    """Reference launch (:140-212): model + snapshot + Diffusion + tiler.  The image file I/O of the reference
    (PIL / torchvision.transforms) is outside the hot path: `--img_lr_path` takes a `.pt` / `.npy` tensor (C,H,W) or
    (1,C,H,W) in [0,1], `--destination_path` receives a `.pt` tensor."""
    import os

    from .colorfix import cli_color_fix
    from .train_diffusion_superres import Diffusion, cli_sampling_steps
    from .UNet_model_superres import Residual_Attention_UNet_superres
    device = args.device
    if args.UNet_type.lower() != "residual attention unet":
        raise ValueError("The UNet type must be Residual Attention UNet")
    model = Residual_Attention_UNet_superres(args.inp_out_channels, args.inp_out_channels, device).to(device)
    print(f"You are using {args.UNet_type} model")
    path = args.img_lr_path
    img_lr = torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path)
    img_lr = img_lr.float()
    if img_lr.dim() == 3:
        img_lr = img_lr.unsqueeze(0)
    img_lr = img_lr.to(device)
    diffusion = Diffusion(noise_schedule=args.noise_schedule, model=model,
                          snapshot_path=os.path.join(args.snapshot_folder_path, args.snapshot_name),
                          noise_steps=args.noise_steps, beta_start=1e-4, beta_end=0.02,
                          magnification_factor=args.magnification_factor, device=device,
                          image_size=args.model_input_size, model_name=args.model_name,
                          Degradation_type=args.Degradation_type, multiple_gpus=False, ema_smoothing=False)
    tiler = split_aggregation_sampling(img_lr, args.patch_size, args.stride, args.magnification_factor, diffusion, device)
    final_pred = tiler.aggregation_sampling(sampling_steps=cli_sampling_steps(args),
                                            eta=getattr(args, "eta", 0.0),
                                            aggregation=getattr(args, "aggregation", "final"),
                                            **cli_color_fix(args))
    torch.save(final_pred.squeeze(0).cpu(), args.destination_path)


def build_arg_parser():
    """The reference's flags, verbatim (:217-231), the DDIM flags, --aggregation and the colour-correction flags."""
    import argparse

    from .colorfix import add_color_fix_args
    from .train_diffusion_superres import add_sampling_args, add_solver_args
    p = argparse.ArgumentParser(description=" ")
    p.add_argument("--noise_schedule", type=str, default="cosine")
    p.add_argument("--snapshot_name", type=str, default="snapshot.pt")
    p.add_argument("--noise_steps", type=int, default=1500)
    p.add_argument("--model_input_size", type=int, default=512)
    p.add_argument("--model_name", type=str)
    p.add_argument("--UNet_type", type=str)
    p.add_argument("--Degradation_type", type=str)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--magnification_factor", type=int)
    p.add_argument("--inp_out_channels", type=int, default=3)
    p.add_argument("--patch_size", type=int, default=64)
    p.add_argument("--stride", type=int, default=32)
    p.add_argument("--destination_path", type=str)
    p.add_argument("--img_lr_path", type=str)
    add_sampling_args(p)
    add_solver_args(p)
    p.add_argument("--aggregation", type=str, choices=("final", "per_step"), default="final",
                   help="final: independent tile chains blended once (the reference); per_step: one joint chain of the "
                        "whole scene, the tiles' noise predictions blended at every reverse step")
    add_color_fix_args(p)
    return p


if __name__ == "__main__":
    import os
    a = build_arg_parser().parse_args()
    a.snapshot_folder_path = os.path.join(os.curdir, "models_run", a.model_name, "weights")
    launch(a)
