"""Drop-in `Diffusion` / `launch` / CLI of reference train_diffusion_SAR_TO_NDVI.py on the gfx950 kernels.

Same arithmetic as the super-resolution Diffusion (the reference's two files differ only in the model call,
`model(x_t, t, SAR_img)`, and in the absence of magnification / degradation arguments), so this class reuses the
schedules, q-sample, reverse chain, snapshots and training loop of `train_diffusion_superres.Diffusion` and overrides what
differs: constructor (:80-123), the conditioning image and model call of `sample` (:204-249) and the model call of the loop
bodies (:373-388, :455-470).  `launch` and the CLI are the shared launcher pieces (launcher.py) and parser base and train flags
(cli.py) around this file's dataset, model and two flags.
"""
import os

import torch
import torch.nn as nn

from . import dist as drs_dist
from .augment import add_augment_args
from .cli import (add_finetune_args, add_nodata_args, add_prediction_args, add_train_args, base_arg_parser,  # noqa: F401 - re-exported
                  check_objective_args, check_train_args)
from .launcher import launch_device, make_loaders, save_final_samples, train_model
from .sampling import _repeat_members, asks_for_known_pixels, check_inpaint_args, check_sampling_args
from .train_diffusion_superres import Diffusion as _SuperresDiffusion
from .UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI


class Diffusion(_SuperresDiffusion):
    def __init__(self, noise_schedule: str, model: nn.Module, snapshot_path: str, noise_steps=1000, beta_start=1e-4,
                 beta_end=0.02, device="cuda", image_size=224, model_name="SAR_TO_NDVI", multiple_gpus=False,
                 ema_smoothing=False, prediction="eps", x0_clip=None, x0_threshold=None, zero_terminal_snr=False):
        super().__init__(noise_schedule, model, snapshot_path, noise_steps=noise_steps, beta_start=beta_start,
                         beta_end=beta_end, device=device, magnification_factor=1, image_size=image_size,
                         model_name=model_name, Degradation_type="DownBlur", multiple_gpus=multiple_gpus,
                         ema_smoothing=ema_smoothing, prediction=prediction, x0_clip=x0_clip,
                         x0_threshold=x0_threshold, zero_terminal_snr=zero_terminal_snr)
        del self.magnification_factor, self.Degradation_type  # attributes the reference's SAR Diffusion does not have

    def _predict(self, net, x_t, t, cond):
        return net(x_t, t, cond)

    def sample(self, n, model, SAR_img, NDVI_channels=1, generate_video=False, noise_source=None, sampling_steps=None,
               eta=0.0):
        """Reference :204-249.  One (SAR_channels, S, S) image conditions all n chains; its encoder branch is computed
        once per chain instead of once per step; a 4-D batch of n images conditions one chain each.  `noise_source(i, shape)`, `sampling_steps` and `eta` as in the
        super-resolution sampler."""
        return self._sample(n, model, SAR_img, NDVI_channels, generate_video, noise_source, sampling_steps, eta)

    def sample_known(self, n, model, SAR_img, known, known_mask, NDVI_channels=1, resample=1, jump=1, generate_video=False,
                     noise_source=None, sampling_steps=None, eta=0.0):
        """`sample` with known NDVI pixels, as in the super-resolution `sample_known`: the pixels that are valid (no cloud or
        shadow over them) are kept and only the others are sampled."""
        asks_for_known_pixels(known, known_mask, resample, jump, required=True)
        return self._sample(n, model, SAR_img, NDVI_channels, generate_video, noise_source, sampling_steps, eta, known,
                            known_mask, resample, jump)

    def sample_ensemble(self, n_members, model, SAR_img, NDVI_channels=1, member_batch=None, sampling_steps=None, eta=0.0,
                        noise_source=None, known=None, known_mask=None, resample=1, jump=1):
        """`n_members` >= 2 NDVI samples per SAR image, (n_members, B, NDVI_channels, S, S), for `SAR_img` (B, SAR_channels, S, S)
        or one (SAR_channels, S, S) image (B = 1): the super-resolution `sample_ensemble` - chunks of `member_batch` members,
        each one `sample` (with `known` / `known_mask`: `sample_known`) call on the repeated SAR batch."""
        sar = SAR_img if SAR_img.dim() == 4 else SAR_img.unsqueeze(0)
        args = {"NDVI_channels": NDVI_channels, "noise_source": noise_source, "sampling_steps": sampling_steps, "eta": eta}
        return self._sample_members(n_members, member_batch, sar.shape[0], lambda m: self._ensemble_chunk(
            m * sar.shape[0], (model, sar.repeat(m, 1, 1, 1)), _repeat_members(known, m), _repeat_members(known_mask, m),
            resample, jump, args))

    def _sample(self, n, model, SAR_img, NDVI_channels, generate_video, noise_source, sampling_steps, eta, known=None,
                known_mask=None, resample=1, jump=1):
        check_sampling_args(self.noise_steps, sampling_steps, eta)
        check_inpaint_args((n, NDVI_channels, self.image_size, self.image_size), known, known_mask, resample, jump)
        if SAR_img.dim() == 4:
            # one SAR image per chain, (n, SAR_channels, S, S): what `evaluate` samples a validation batch with
            if SAR_img.shape[0] != n:
                raise RuntimeError(f"sample: a batch of {SAR_img.shape[0]} SAR images for n={n} chains")
            SAR_img = SAR_img.to(self.device).contiguous()
        else:
            SAR_img = SAR_img.to(self.device).unsqueeze(0).contiguous()
        return self._sample_chain(
            model, (n, NDVI_channels, self.image_size, self.image_size),
            lambda engine, x, t, first: engine.forward(x, t, SAR_img, 1, reuse_cond=not first, check_weights=first),
            table_rows=n, generate_video=generate_video, noise_source=noise_source, sampling_steps=sampling_steps, eta=eta,
            known=known, known_mask=known_mask, resample=resample, jump=jump)

    def evaluate(self, model, loader, n_images=None, sampling_steps=None, eta=0.0, noise_source=None, known_mask_fn=None,
                 resample=1, jump=1, ensemble=None, member_batch=None, nodata=None):
        """PSNR / SSIM (and the spectral angle when NDVI has several bands) of `sample`'s output against the NDVI truth over
        the (SAR, NDVI) batches of `loader`: the super-resolution `evaluate` without a magnification, hence without ERGAS, and
        without a bicubic baseline; `known_mask_fn` / `resample` / `jump` as there ("psnr_unknown").
        Returns {"model": {metric: mean}, "per_image": {"model": {metric: [...]}}, "n": N}; with `ensemble=N` (and
        `member_batch`) also "member" and "ensemble", as the super-resolution `evaluate` does.  `nodata` as there: the scores
        are over the valid pixels of the NDVI truth, and "valid_fraction" is added."""
        self._check_evaluate_nodata(nodata, ensemble, known_mask_fn)
        sample, members = self._evaluate_samplers(model, "NDVI_channels", sampling_steps, eta, noise_source, known_mask_fn,
                                                  resample, jump, ensemble, member_batch)
        return self._evaluate(model, loader, n_images, {"model": sample}, None, members, nodata)


class SyntheticSarNdviDataset(torch.utils.data.Dataset):
    """Seeded (SAR_img, NDVI_img) pairs with the shapes `get_data_SAR_TO_NDVI` yields (reference utils.py):
    `--dataset_path synthetic[:N]`."""

    def __init__(self, length, sar_channels, ndvi_channels, image_size, seed=0):
        from . import synthetic
        self.sar = synthetic.tensor_uniform("synthetic.sar", (length, sar_channels, image_size, image_size), seed)
        self.ndvi = synthetic.tensor_uniform("synthetic.ndvi", (length, ndvi_channels, image_size, image_size), seed)

    def __len__(self):
        return self.sar.shape[0]

    def __getitem__(self, i):
        return self.sar[i], self.ndvi[i]


def synthetic_datasets(args):
    """(train, validation) seeded datasets of `--dataset_path synthetic[:N]`."""
    spec = str(args.dataset_path or "")
    length = int(spec.split(":")[1]) if ":" in spec else 4 * args.batch_size
    return (SyntheticSarNdviDataset(length, args.SAR_channels, args.NDVI_channels, args.image_size, seed=1),
            SyntheticSarNdviDataset(max(length // 4, 1), args.SAR_channels, args.NDVI_channels, args.image_size, seed=2))


def folder_feed(args, device, split, rank=0, world_size=1, limit=None, fixed=None):
    """The device feed of `<dataset_path>/<split>/{sar,opt}` (reference :567-571: split 'train' or 'test'), checked against the
    flags: the reference resizes nothing here, so the files must have --image_size and the models' band counts.  With
    --scene_size P the files must be P x P and the items are --image_size windows (augment.py); `fixed` (default: every split but
    'train', and the `limit` feed of the final sampling): the centre windows, no augmentation."""
    from .augment import feed_kwargs, scene_size
    from .feeds import DeviceSarNdviFeed, load_sar_ndvi_folder
    size = scene_size(args)
    flag = "--scene_size" if getattr(args, "scene_size", None) is not None else "--image_size"
    if fixed is None:
        fixed = split != "train" or limit is not None
    root = os.path.join(args.dataset_path, split)
    if not os.path.isdir(os.path.join(root, "sar")) or not os.path.isdir(os.path.join(root, "opt")):
        raise FileNotFoundError(f"--dataset_path {args.dataset_path!r}: expected the folders train/sar, train/opt, test/sar and "
                                f"test/opt (or synthetic[:N]); {root} lacks sar/ or opt/")
    sar, ndvi = load_sar_ndvi_folder(root, getattr(args, "data_format", "torch"), rank, world_size, limit,
                                     nodata=getattr(args, "nodata", None))
    for what, t, bands_flag, want in (("sar", sar, "--SAR_channels", args.SAR_channels),
                                      ("opt", ndvi, "--NDVI_channels", args.NDVI_channels)):
        if t.shape[1] != want:
            raise ValueError(f"the images of {root}/{what} have {t.shape[1]} bands, {bands_flag} is {want}")
        if tuple(t.shape[2:]) != (size, size):
            raise ValueError(f"the images of {root}/{what} are {t.shape[2]} x {t.shape[3]}, {flag} is {size} "
                             "(this dataset is not resized)")
    return DeviceSarNdviFeed(sar.to(device), ndvi.to(device), args.batch_size, shuffle=True, **feed_kwargs(args, rank, fixed))


def launch(args):
    """Reference launch (:505-633): model + Diffusion + train + final sampling.  `--dataset_path` is the reference's folder
    (`<path>/train/{sar,opt}`, `<path>/test/{sar,opt}`, :567-571: read once into a cache on the device, batches gathered there) or
    `synthetic[:N]` (seeded pairs)."""
    if args.UNet_type.lower() != "residual attention unet":
        raise ValueError("The UNet type must be Residual Attention UNet")
    device = launch_device(args)
    folder = not str(args.dataset_path or "").startswith("synthetic")
    if folder:
        r, wsz = (drs_dist.rank(), drs_dist.world_size()) if args.multiple_gpus else (0, 1)
        train_loader = folder_feed(args, device, "train", r, wsz)  # with --multiple_gpus: this rank's shard only
        val_loader = folder_feed(args, device, "test", r, wsz)
    else:
        train_dataset, val_dataset = synthetic_datasets(args)
        train_loader, val_loader = make_loaders(args, train_dataset, val_dataset)
    model = Residual_Attention_UNet_SAR_TO_NDVI(args.SAR_channels, args.NDVI_channels, device).to(device)
    # (--nodata: the folder loader has turned every no-data pixel into NaN, so the run masks by the NaN rule; the seeded pairs
    #  are not rewritten: the rule is applied to the batches as it stands)
    nodata = getattr(args, "nodata", None)
    diffusion = train_model(args, Diffusion, model, device, train_loader, val_loader,
                            nodata=True if folder and nodata is not None else nodata)
    if folder:
        if r != 0:
            return  # one rank samples and writes the results, as in the super-resolution launch
        # train_dataset[0..4] of the WHOLE sorted folder (reference :622-626), whatever this rank's shard holds
        first = folder_feed(args, device, "train", limit=5)
        final_sar = [first.item(i)[0] for i in range(first.sar.shape[0])]
    else:
        final_sar = [train_dataset[i][0] for i in range(min(5, len(train_dataset)))]

    def sample(sar_img, **ddim):
        return diffusion.sample(n=1, model=model, SAR_img=sar_img, NDVI_channels=args.NDVI_channels,
                                generate_video=args.generate_video, **ddim)
    save_final_samples(args, sample, final_sar, "SAR_TO_NDVI_results.pt")


def build_arg_parser():
    """`base_arg_parser` and the SAR -> NDVI flags of the reference (:646-663)."""
    p = base_arg_parser()
    p.add_argument("--SAR_channels", type=int, default=2)
    p.add_argument("--NDVI_channels", type=int, default=1)
    return p


def train_arg_parser():
    """The trainer's command line: `build_arg_parser` and `--data_format`, an argument of the reference's dataset class
    (utils.py:54) that its launch leaves at the default."""
    p = build_arg_parser()
    p.add_argument("--data_format", type=str, default="torch", choices=("torch", "numpy"),
                   help="file format of a dataset folder: .pt tensors (the reference dataset's default) or .npy arrays")
    return p


def train_main_parser():
    """`train_arg_parser`, the crop / augmentation flags (augment.add_augment_args) and the optimizer / resume and objective
    flags (cli.add_train_args): what `main` parses."""
    p = train_arg_parser()
    add_augment_args(p)
    return add_nodata_args(add_finetune_args(add_prediction_args(add_train_args(p), in_help=False)), in_help=False)


def main(argv=None):
    parser = train_main_parser()
    args = check_train_args(parser, parser.parse_args(argv))
    args.snapshot_folder_path = os.path.join(os.curdir, "models_run", args.model_name, "weights")
    launch(args)


if __name__ == "__main__":
    main()
