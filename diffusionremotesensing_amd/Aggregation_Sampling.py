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

Not in the reference either: known pixels (`known` / `known_mask`, RePaint as in `Diffusion.sample_known`) in both modes, and
a sampled state whose channels and data range are not the conditioning image's (`out_channels`, `clamp`), so that the
SAR -> NDVI model fills the clouded part of a whole NDVI scene.
"""
from math import exp, pi, sqrt

import numpy as np
import torch

from . import dist as drs_dist
from . import hip_ops


# tiles per sampling chain (per rank): bounds the plan workspace (~0.1 GB per 256x256 tile) independently of the scene size
TILE_BATCH = 16


_WEIGHT_TABLES = {}  # (tile width, tile height, device) -> the Gaussian tile weights on the device


class split_aggregation_sampling:
    def __init__(self, img_lr, patch_size, stride, magnification_factor, diffusion_model, device, *, out_channels=None,
                 clamp=(0.0, 1.0)):
        """`out_channels`: channels of the sampled state (None: those of `img_lr`, the super-resolution case; NDVI_channels
        with a SAR -> NDVI `Diffusion`, a SAR scene as `img_lr` and `magnification_factor=1`).  `clamp`: the (lo, hi) range
        `aggregation_sampling` clamps to, None for none (NDVI lives in [-1, 1])."""
        assert stride <= patch_size
        self.img_lr = img_lr
        self.patch_size = patch_size
        self.stride = stride
        self.magnification_factor = magnification_factor
        self.diffusion_model = diffusion_model
        self.device = device
        self.model = diffusion_model.model
        batch_size, channels, height, width = img_lr.shape
        self.out_channels = channels if out_channels is None else int(out_channels)
        self.clamp = None if clamp is None else hip_ops._clamp_args(clamp, "split_aggregation_sampling")[1:]
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
        # (uploaded once per tile size and device: an upload from pageable memory makes the host wait for the current stream)
        key = (tile_width, tile_height, str(self.device))
        weights = _WEIGHT_TABLES.get(key)
        if weights is None:
            weights = _WEIGHT_TABLES[key] = torch.tensor(np.outer(y_probs, x_probs)).to(torch.float32).to(self.device)
        return torch.tile(weights, (nbatches, 3, 1, 1))

    def _scene_size(self):
        batch_size, channels, height, width = self.img_lr.shape
        return height * self.magnification_factor, width * self.magnification_factor

    def check_known(self, sampling_steps, known, known_mask, resample=1, jump=1):
        """ValueError for a known-pixel request on this scene (checked before the engine is touched): `known` that is not
        (out_channels, Hs, Ws), a `known_mask` that is not (Hs, Ws) or (1 | out_channels, Hs, Ws), one without the other,
        `resample` / `jump` without `known`, or a "dpmpp_2m" plan with known pixels."""
        from .sampling import check_inpaint_args, check_solver_known
        Hs, Ws = self._scene_size()
        C = self.out_channels
        if known is not None and tuple(known.shape) != (C, Hs, Ws):
            raise ValueError(f"known {tuple(known.shape)} must be the scene {(C, Hs, Ws)}")
        if known_mask is not None and tuple(known_mask.shape) not in ((Hs, Ws), (1, Hs, Ws), (C, Hs, Ws)):
            raise ValueError(f"known_mask {tuple(known_mask.shape)} must be {(Hs, Ws)} or (1 | {C}, {Hs}, {Ws})")
        check_inpaint_args((1, C, Hs, Ws), known, known_mask, resample, jump)
        check_solver_known(sampling_steps, known, known_mask)

    def known_tiles(self, known, known_mask):
        """The crops of `known` (C, Hs, Ws) and `known_mask` ((Hs, Ws) or (1 | C, Hs, Ws)) at the tiles' windows
        (`patches_sr_infos`): (n, C, S, S) and (n, 1 | C, S, S), the per-chain tensors of `sample_known`."""
        mask = known_mask if known_mask.dim() == 3 else known_mask.unsqueeze(0)
        return (torch.stack([known[:, y0:y1, x0:x1] for (y0, y1, x0, x1) in self.patches_sr_infos]),
                torch.stack([mask[:, y0:y1, x0:x1] for (y0, y1, x0, x1) in self.patches_sr_infos]))

    @staticmethod
    def _chunk(t, c0, c1, size):
        """t[c0:c1], padded to `size` entries with repeats of its last one (a fixed-size chunk of tiles)."""
        t_c = t[c0:c1]
        if size > c1 - c0:
            t_c = torch.cat([t_c, t_c[-1:].expand(size - (c1 - c0), -1, -1, -1)], dim=0).contiguous()
        return t_c

    def sample_tiles(self, noise_source=None, sampling_steps=None, eta=0.0, known=None, known_mask=None, resample=1, jump=1):
        """Sample every tile: (n_tiles, C, S, S) on this rank's device.  One batched chain (sharded over the
        ranks of an initialised process group); `sampling_steps` / `eta` select a DDIM chain (`Diffusion.sample`).
        With `known` / `known_mask` of scene size (`check_known`) every chunk is a `sample_known` call on the tiles' crops of
        both (`known_tiles`), chunked, padded and sharded like the LR tiles; `resample` / `jump` as there, and
        `noise_source(tile, i, shape)` is asked at that chain's draws."""
        d = self.diffusion_model
        self.check_known(sampling_steps, known, known_mask, resample, jump)
        lr = torch.cat([p[:1] for p in self.patches_lr], dim=0).to(self.device).contiguous()  # (n, C, ps, ps)
        n = lr.shape[0]
        lo, hi = drs_dist.shard_range(n) if drs_dist.world_size() > 1 else (0, n)
        kn = mk = None
        if known is not None:
            kn, mk = self.known_tiles(known.to(self.device), known_mask.to(self.device))
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
        S = self.patch_size * self.magnification_factor
        outs = []
        for c0 in range(lo, hi, chunk):
            c1 = min(c0 + chunk, hi)
            take = c1 - c0
            size = take if (hi - lo) <= chunk else chunk  # a scene smaller than one chunk runs at its own size
            lr_c = self._chunk(lr, c0, c1, size)
            csrc = None
            if src is not None:
                def csrc(i, shape, c0=c0, take=take):
                    real = src(i, (take,) + tuple(shape[1:]), lo=c0)
                    if shape[0] > take:
                        real = torch.cat([real, real[-1:].expand(shape[0] - take, -1, -1, -1)], dim=0)
                    return real
            # the channel count goes positionally: `input_channels` of one sampler is `NDVI_channels` of the other
            if kn is None:
                out_c = d.sample(size, self.model, lr_c, self.out_channels, generate_video=False, noise_source=csrc, **ddim)
            else:
                out_c = d.sample_known(size, self.model, lr_c, self._chunk(kn, c0, c1, size), self._chunk(mk, c0, c1, size),
                                       self.out_channels, resample=resample, jump=jump, generate_video=False,
                                       noise_source=csrc, **ddim)
            outs.append(out_c[:take])
        mine = torch.cat(outs, dim=0) if outs else lr.new_zeros((0, self.out_channels, S, S))
        if drs_dist.world_size() > 1:
            mine = drs_dist.gather_shards(mine, n)
        return mine

    def sample_scene(self, noise_source=None, sampling_steps=None, eta=0.0, known=None, known_mask=None, resample=1, jump=1):
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
        The loop is `run_reverse_chain`: the fault-word reads and the range-fault roll-back act on the scene state.
        Known pixels.  `known` (C, Hs, Ws, in the model's data range, used as given) with `known_mask` ((Hs, Ws) or
        (1 | C, Hs, Ws); bool, uint8 or {0, 1} float, nonzero = known) keeps those pixels of the scene (RePaint, as
        `Diffusion.sample_known` does per image): the moves are `chain_moves(..., resample, jump)`; a reverse move is the same
        gather / forwards / one `blend_step_`, which then also replaces the known elements of the scene state by `known`
        forward-noised to the level reached (`known` itself at level 0) with the move's draw - `noise_source(i, scene shape)`,
        drawn iff the move ends above level 0, whatever eta is; a forward jump to level t is one `renoise_` of the scene state
        with `noise_source(t, scene shape)`.  The known pixels of the returned scene are `known`, exactly.  Memory: `known` and
        its uint8 mask, once, at scene size (4 + 1 bytes per element read per move).  ValueError as `check_known`."""
        from .sampling import check_sampling_args
        d = self.diffusion_model
        if getattr(d, "zero_terminal_snr", False):
            raise ValueError("aggregation='per_step' cannot run on a zero_terminal_snr schedule: its per-tile conversion of the "
                             "prediction to eps is 0 / 0 at the terminal level (alpha_hat == 0); use aggregation='final'")
        check_sampling_args(d.noise_steps, sampling_steps, eta)
        self.check_known(sampling_steps, known, known_mask, resample, jump)
        if drs_dist.world_size() > 1:
            raise NotImplementedError(
                "aggregation='per_step' runs on one rank: the joint chain would need an all-gather of eps and a shared "
                "noise draw per step; use aggregation='final', which shards its independent tile chains over the ranks")
        batch_size, _, height, width = self.img_lr.shape
        channels = self.out_channels
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
        # what the network predicts (`Diffusion(prediction=, x0_clip=)`): its output becomes eps here, chunk by chunk against the
        # tiles it saw, since the chain's state is the scene; with "eps" and no clip nothing is launched
        # with `x0_threshold` the clamp is dynamic thresholding, per tile: the image the network saw
        from .sampling import check_prediction, check_threshold, converts_prediction
        prediction, x0_clip = check_prediction(getattr(d, "prediction", "eps"), getattr(d, "x0_clip", None))
        x0_threshold = check_threshold(getattr(d, "x0_threshold", None), x0_clip)
        dynamic = {"x0_threshold": x0_threshold} if x0_threshold is not None else {}
        convert = prediction != "eps" or x0_clip is not None

        def predict(engine, x, t, first):
            for j, c0 in enumerate(starts):
                hip_ops.gather_tiles(x[0], origins, S, out=x_tiles, first=c0, count=size)
                engine.forward(x_tiles, t, lr_chunks[j], m, reuse_cond=single and not first,
                               check_weights=first and j == 0, out=eps_buf[c0:c0 + size])
                if convert:
                    hip_ops.pred_to_eps_(eps_buf[c0:c0 + size], x_tiles, t, d.alpha_hat, prediction, x0_clip, **dynamic)
            return eps_buf
        if convert:
            converts_prediction(predict)

        def update(x, eps, noise, i, i_prev, hist=None, t_q=-1, known=None, known_mask=None):
            kept = {"known": known[0], "known_mask": known_mask[0]} if known is not None else {}
            hip_ops.blend_step_(x[0], eps, origins, weight, noise[0] if noise is not None else None, i,
                                alpha_hat=d.alpha_hat, alpha=d.alpha, beta=d.beta, t_prev=i_prev, eta=eta,
                                uncovered=uncovered, hist=hist[0] if hist is not None else None, t_q=t_q, **kept)

        kept = {"known": known, "known_mask": known_mask, "resample": resample, "jump": jump} if known is not None else {}
        x = d._sample_chain(self.model, (1, channels, Hs, Ws), predict, table_rows=size, generate_video=False,
                            noise_source=noise_source, sampling_steps=sampling_steps, eta=eta, update=update, **kept)
        if int(uncovered.item()) != 0:
            raise AssertionError("aggregation: some scene pixels are covered by no tile (pixel_count == 0)")
        return x[0]

    def aggregation_sampling(self, noise_source=None, sampling_steps=None, eta=0.0, aggregation="final", color_fix=None,
                             color_fix_levels=5, known=None, known_mask=None, resample=1, jump=1, lr_consistency=None):
        """Reference :76-116 (`sampling_steps` / `eta`: every tile runs a DDIM chain).  `aggregation`: "final" (the
        reference: independent tile chains, blended once; `noise_source(tile, i, shape)`) or "per_step" (`sample_scene`:
        one joint chain, blended at every step; `noise_source(i, scene_shape)`), clamped to [0, 1] (the constructor's `clamp`).
        `color_fix`: None (the default: nothing changes), "wavelet" (with `color_fix_levels`) or "adain" - the finished, clamped
        scene is corrected once as a whole, never per tile, against the bicubic up-sampling of img_lr's first image
        (`colorfix.color_fix`) and clamped to [0, 1] again.
        `known` / `known_mask` of scene size (`sample_scene`), with `resample` / `jump`, keep those pixels in either mode: the
        tiles' chains (`sample_tiles`) or the joint chain keep them at every step, and the known pixels of the blended scene are
        `known` under the clamp, exactly (in the final mode one `aggregate_tiles(..., known=, known_mask=)`).
        `lr_consistency` (a consistency.LRConsistency; super-resolution only) projects the finished scene once, as a whole, onto
        the scenes the degradation maps to img_lr's first image (`consistency.project` with an operator of scene size, (H m, W m)
        -> (H, W)): in either mode, after `color_fix` and before the last clamp.  It does not reach into the chains: in the final
        mode the tiles' chains follow `diffusion_model.lr_consistency`, each against its own LR tile - a cropped LR image, whose
        borders the operator treats as the image's edge - and the per-step chain takes none (`sample_chain` refuses the pair)."""
        if aggregation not in ("final", "per_step"):
            raise ValueError(f"aggregation={aggregation!r} must be 'final' or 'per_step'")
        fix = self._lr_project(lr_consistency, self._color_fix(color_fix, color_fix_levels))
        self.check_known(sampling_steps, known, known_mask, resample, jump)
        batch_size, channels, height, width = self.img_lr.shape
        m = self.magnification_factor
        kept = {"known": known, "known_mask": known_mask, "resample": resample, "jump": jump} if known is not None else {}
        if aggregation == "per_step":
            out = fix(self._clamp(self.sample_scene(noise_source, sampling_steps=sampling_steps, eta=eta, **kept)))
            return out.unsqueeze(0).expand(batch_size, -1, -1, -1).contiguous()
        tiles = self.sample_tiles(noise_source, sampling_steps=sampling_steps, eta=eta, **kept)
        origins = [(info[0], info[2]) for info in self.patches_sr_infos]
        blend = {"clamp": self.clamp}
        if known is not None:
            from .sampling import known_tensors
            kn, mk = known_tensors((1, self.out_channels, height * m, width * m), known, known_mask, tiles.device)
            blend.update(known=kn[0], known_mask=mk[0])
        out = fix(hip_ops.aggregate_tiles(tiles, origins, self.weight[0, 0].contiguous(), height * m, width * m, **blend))
        # the reference broadcasts the single chain of each tile over the batch dimension of img_lr
        return out.unsqueeze(0).expand(batch_size, -1, -1, -1).contiguous()

    def _clamp(self, scene):
        return scene if self.clamp is None else torch.clamp(scene, self.clamp[0], self.clamp[1])

    def _lr_project(self, request, fix):
        """`fix` followed by the scene's LR projection and the clamp; `fix` itself without a request.  The operator and its
        projector are made here, before anything is sampled (ValueError for a request this scene does not take)."""
        from .consistency import check_lr_consistency, project
        if check_lr_consistency(request) is None:
            return fix
        Hs, Ws = self._scene_size()
        batch_size, channels, height, width = self.img_lr.shape
        if channels != self.out_channels:
            raise ValueError(f"lr_consistency: the conditioning has {channels} bands, the scene {self.out_channels}: it is no "
                             "degraded copy of the scene (super-resolution only)")
        projector = request.operator_for(self.diffusion_model, (Hs, Ws), lr_hw=(height, width)).projector(request.damping, self.device)

        def projected(scene):
            scene = fix(scene)
            lr = self.img_lr[:1].to(scene.device, torch.float32).contiguous()
            return self._clamp(project(scene.unsqueeze(0).contiguous(), lr, projector, request.strength)[0])
        return projected

    def _color_fix(self, method, levels):
        """f(clamped scene (C, Hs, Ws)) -> the scene `aggregation_sampling` returns: the identity without a method (checked
        here, before anything is sampled); the corrected scene is clamped like the sampled one (the constructor's `clamp`)."""
        if method is None:
            return lambda scene: scene
        from .colorfix import color_fix, fix_levels
        levels = fix_levels(method, levels)

        def fix(scene):
            lr = self.img_lr[:1].to(scene.device, torch.float32).contiguous()
            fixed = color_fix(scene.unsqueeze(0), lr, magnification_factor=self.magnification_factor, method=method,
                              levels=levels)
            return self._clamp(fixed[0])
        return fix


def _load_tensor(path):
    """A `.pt` / `.npy` tensor file, as `--img_lr_path` takes it."""
    return torch.from_numpy(np.load(path)) if path.endswith(".npy") else torch.load(path)


def cli_clamp(args):
    """The tiler's `clamp` of the command line: `--clamp none` or `LO,HI`; unset it is [0, 1] for super-resolution and none
    for SAR -> NDVI (whose data range the reference leaves to the dataset)."""
    text = getattr(args, "clamp", None)
    if text is None:
        return None if getattr(args, "task", "superres") == "sar_to_ndvi" else (0.0, 1.0)
    if text.strip().lower() == "none":
        return None
    parts = text.split(",")
    if len(parts) != 2:
        raise ValueError(f"--clamp {text!r} must be 'none' or 'LO,HI'")
    return float(parts[0]), float(parts[1])


def launch(args):
    """Reference launch (:140-212): model + snapshot + Diffusion + tiler.  The image file I/O of the reference
    (PIL / torchvision.transforms) is outside the hot path: `--img_lr_path` takes a `.pt` / `.npy` tensor (C,H,W) or
    (1,C,H,W) in [0,1] - or a uint16 `.npy` of digital numbers, normalised with the snapshot's band ranges or `--data_range` -,
    `--destination_path` receives a `.pt` tensor (`--out_u16`: a uint16 `.npy` of digital numbers).  `--task sar_to_ndvi` builds the SAR -> NDVI model and
    `Diffusion` instead (`--SAR_channels`, `--NDVI_channels`; `--img_lr_path` is then the SAR scene and
    `--magnification_factor` must be 1); `--known_path` / `--known_mask_path` hold the known scene (C_out,Hs,Ws) and its mask."""
    import os

    from .colorfix import cli_color_fix
    from .cli import cli_consistency, cli_prediction, cli_sampling_steps, cli_threshold, cli_ztsnr, set_guidance_rescale
    device = args.device
    task = getattr(args, "task", "superres")
    if args.UNet_type.lower() != "residual attention unet":
        raise ValueError("The UNet type must be Residual Attention UNet")
    snapshot_path = os.path.join(args.snapshot_folder_path, args.snapshot_name)
    if task == "sar_to_ndvi":
        from .train_diffusion_SAR_TO_NDVI import Diffusion
        from .UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
        if args.magnification_factor != 1:
            raise ValueError(f"--task sar_to_ndvi samples at the SAR scene's size: --magnification_factor must be 1, got "
                             f"{args.magnification_factor}")
        model = Residual_Attention_UNet_SAR_TO_NDVI(args.SAR_channels, args.NDVI_channels, device).to(device)
        diffusion = Diffusion(noise_schedule=args.noise_schedule, model=model, snapshot_path=snapshot_path,
                              noise_steps=args.noise_steps, beta_start=1e-4, beta_end=0.02, device=device,
                              image_size=args.model_input_size, model_name=args.model_name, multiple_gpus=False,
                              ema_smoothing=False, **cli_prediction(args), **cli_threshold(args), **cli_ztsnr(args))
        out_channels = args.NDVI_channels
    elif task == "superres":
        from .train_diffusion_superres import Diffusion
        from .UNet_model_superres import Residual_Attention_UNet_superres
        model = Residual_Attention_UNet_superres(args.inp_out_channels, args.inp_out_channels, device).to(device)
        # an MTF run (mtf.py): --mtf_nyquist, else the snapshot's MTF_NYQUIST; neither: whatever --Degradation_type says
        from . import mtf
        nyquist = mtf.resolve_nyquist(args, snapshot_path, args.inp_out_channels)
        degradation = {"Degradation_type": args.Degradation_type} if nyquist is None else \
            {"Degradation_type": "MTF", "mtf_nyquist": nyquist}
        diffusion = Diffusion(noise_schedule=args.noise_schedule, model=model, snapshot_path=snapshot_path,
                              noise_steps=args.noise_steps, beta_start=1e-4, beta_end=0.02,
                              magnification_factor=args.magnification_factor, device=device,
                              image_size=args.model_input_size, model_name=args.model_name,
                              multiple_gpus=False, ema_smoothing=False, **degradation,
                              **cli_prediction(args), **cli_threshold(args), **cli_ztsnr(args))
        out_channels = None
    else:
        raise ValueError(f"--task {task!r} must be 'superres' or 'sar_to_ndvi'")
    set_guidance_rescale(diffusion, args)
    consistent = cli_consistency(args)
    if consistent["lr_consistency"] is not None:
        if task != "superres":
            raise ValueError("--lr_consistency belongs to --task superres: only its conditioning is a degraded copy of the scene")
        if getattr(args, "aggregation", "final") == "final":  # (the per-step chain takes none: the finished scene is projected)
            diffusion.lr_consistency = consistent["lr_consistency"]
    print(f"You are using {args.UNet_type} model")
    img_lr, data_range = _load_tensor(args.img_lr_path), None
    if img_lr.dtype == torch.uint16 or getattr(args, "out_u16", False):
        # 16-bit digital numbers (radiometry.py): normalised with --data_range, else with the band ranges in the snapshot
        from . import radiometry
        channels = img_lr.shape[-3] if img_lr.dim() >= 3 else 1
        given = getattr(args, "data_range", None)
        if given is not None:
            kind, *rest = radiometry.parse_data_range(given)
            if kind != "fixed":
                raise ValueError("--data_range auto needs a training cache: the tiler takes LO,HI or LO,HI;LO,HI;...")
            data_range = radiometry.range_table(rest[0], channels)
        else:
            data_range = getattr(diffusion, "snapshot_data_range", None)
            if data_range is None:
                raise ValueError(f"{snapshot_path} holds no DATA_RANGE (it was not trained with --bit_depth 16): give --data_range")
            data_range = radiometry.check_table(data_range, channels)
        if img_lr.dtype == torch.uint16:
            img_lr = torch.from_numpy(radiometry.normalise_host(img_lr.numpy(), data_range, band_axis=img_lr.dim() - 3))
    elif getattr(args, "data_range", None) is not None:
        raise ValueError("--data_range belongs to a uint16 --img_lr_path or to --out_u16")
    img_lr = img_lr.float()
    if img_lr.dim() == 3:
        img_lr = img_lr.unsqueeze(0)
    img_lr = img_lr.to(device)
    kept = {}
    if getattr(args, "known_path", None) or getattr(args, "known_mask_path", None):
        if not (getattr(args, "known_path", None) and getattr(args, "known_mask_path", None)):
            raise ValueError("--known_path and --known_mask_path go together")
        kept = {"known": _load_tensor(args.known_path).float(), "known_mask": _load_tensor(args.known_mask_path)}
    resample, jump = getattr(args, "known_resample", 1), getattr(args, "known_jump", 1)
    if resample != 1 or jump != 1 or kept:
        kept.update(resample=resample, jump=jump)
    tiler = split_aggregation_sampling(img_lr, args.patch_size, args.stride, args.magnification_factor, diffusion, device,
                                       out_channels=out_channels, clamp=cli_clamp(args))
    final_pred = tiler.aggregation_sampling(sampling_steps=cli_sampling_steps(args),
                                            eta=getattr(args, "eta", 0.0),
                                            aggregation=getattr(args, "aggregation", "final"),
                                            **cli_color_fix(args), **kept,
                                            **{k: v for k, v in consistent.items() if v is not None})
    if getattr(args, "out_u16", False):  # the scene as digital numbers, a uint16 .npy (C, H, W)
        from . import radiometry
        final_pred = final_pred if final_pred.dim() == 4 else final_pred.unsqueeze(0)
        dn = radiometry.quantize_u16(final_pred.float().contiguous(), radiometry.device_table(data_range, final_pred.device))
        with open(args.destination_path, "wb") as f:  # (np.save would append .npy to another name)
            np.save(f, dn.squeeze(0).cpu().numpy())
        return
    torch.save(final_pred.squeeze(0).cpu(), args.destination_path)


def build_arg_parser():
    """The reference's flags, verbatim (:217-231), the DDIM flags, --aggregation, the colour-correction flags, the LR-consistency
    flags (`cli.add_consistency_args`), the known-pixel flags, --task / --clamp and --prediction / --x0_clip (the snapshot's prediction; the clip of the x0 implied at every step)."""
    import argparse

    from .colorfix import add_color_fix_args
    from .cli import add_consistency_args, add_prediction_args, add_sampling_args, add_solver_args
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
    add_prediction_args(p)
    p.add_argument("--aggregation", type=str, choices=("final", "per_step"), default="final",
                   help="final: independent tile chains blended once (the reference); per_step: one joint chain of the "
                        "whole scene, the tiles' noise predictions blended at every reverse step")
    add_color_fix_args(p)
    add_consistency_args(p)
    from .mtf import add_mtf_args
    add_mtf_args(p, noise=False)
    p.add_argument("--known_path", type=str, default=None,
                   help=".pt / .npy scene (C_out,Hs,Ws) whose pixels under --known_mask_path are kept (RePaint)")
    p.add_argument("--known_mask_path", type=str, default=None,
                   help=".pt / .npy mask (Hs,Ws) or (1 | C_out,Hs,Ws), nonzero = known")
    p.add_argument("--resample", dest="known_resample", type=int, default=1,
                   help="RePaint resampling rounds per jump (1: none); needs --known_path")
    p.add_argument("--jump", dest="known_jump", type=int, default=1,
                   help="RePaint jump length in chain positions; needs --known_path")
    p.add_argument("--task", type=str, choices=("superres", "sar_to_ndvi"), default="superres",
                   help="sar_to_ndvi: --img_lr_path is a SAR scene, sampled to NDVI at --magnification_factor 1")
    p.add_argument("--SAR_channels", type=int, default=2)
    p.add_argument("--NDVI_channels", type=int, default=1)
    p.add_argument("--data_range", type=str, default=None,
                   help="LO,HI or LO,HI;LO,HI;... : the band ranges a uint16 --img_lr_path .npy (digital numbers) is normalised "
                        "with and --out_u16 writes with; default: the DATA_RANGE of the snapshot (a --bit_depth 16 training run)")
    p.add_argument("--out_u16", action="store_true",
                   help="write --destination_path as a uint16 .npy of digital numbers (C,H,W) under the band ranges")
    p.add_argument("--clamp", type=str, default=None,
                   help="'none' or 'LO,HI' (--clamp=-1,1 for a negative bound): the range of the returned scene; default 0,1 for "
                        "superres, none for sar_to_ndvi")
    return p


if __name__ == "__main__":
    import os
    a = build_arg_parser().parse_args()
    a.snapshot_folder_path = os.path.join(os.curdir, "models_run", a.model_name, "weights")
    launch(a)
