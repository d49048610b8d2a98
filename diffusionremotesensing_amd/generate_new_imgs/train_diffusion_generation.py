"""Drop-in `Diffusion` / `launch` / CLI of reference generate_new_imgs/train_diffusion_generation.py on the gfx950
kernels: class-conditional DDPM with classifier-free guidance.

Overrides what differs from the super-resolution Diffusion it derives from: no conditioning image, the loader yields
(img, label), 10% of the training steps drop the label (:393-394), and the model call of `sample` is a conditional and
(for cfg_scale > 0) an unconditional prediction per step, combined with torch.lerp (:236-239) by the base class's reverse
chain.  `launch` and the CLI are the shared launcher pieces (launcher.py) and parser base and train flags (cli.py) around this
file's datasets (the reference's class-folder tree through the device feed of feeds.py, or seeded images), model and flag.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from .. import dist as drs_dist
from ..augment import add_augment_args
from ..cli import add_finetune_args, add_prediction_args, add_train_args, base_arg_parser, check_objective_args, check_train_args  # noqa: F401 - re-exported
from ..launcher import launch_device, make_loaders, save_final_samples, train_model
from ..sampling import _repeat_members, asks_for_known_pixels, check_inpaint_args, check_sampling_args
from ..train_diffusion_superres import Diffusion as _SuperresDiffusion
from .UNet_model_generation import Residual_Attention_UNet_generation


class Diffusion(_SuperresDiffusion):
    def __init__(self, noise_schedule: str, model: nn.Module, snapshot_path: str, noise_steps=1000, beta_start=1e-4,
                 beta_end=0.02, device="cuda", image_size=224, model_name="generation", multiple_gpus=False,
                 ema_smoothing=False, prediction="eps", x0_clip=None, x0_threshold=None, zero_terminal_snr=False):
        super().__init__(noise_schedule, model, snapshot_path, noise_steps=noise_steps, beta_start=beta_start,
                         beta_end=beta_end, device=device, magnification_factor=1, image_size=image_size,
                         model_name=model_name, Degradation_type="DownBlur", multiple_gpus=multiple_gpus,
                         ema_smoothing=ema_smoothing, prediction=prediction, x0_clip=x0_clip,
                         x0_threshold=x0_threshold, zero_terminal_snr=zero_terminal_snr)
        del self.magnification_factor, self.Degradation_type

    def _split_batch(self, batch):
        """Loader items are (img, label) (:384-386); returned as (conditioning = label, clean image)."""
        return batch[1].to(self.device), batch[0].to(self.device)

    def _train_cond(self, label):
        # 10% of the training and validation steps run unconditionally (:393-394, :466-467); same host RNG call
        return None if np.random.random() < 0.1 else label

    def _predict(self, net, x_t, t, cond):
        return net(x_t, t, cond)

    def _check_nodata(self, loss):
        """The generation trainer has no no-data pixels: its images are decoded RGB files."""
        if self.nodata is not None:
            raise ValueError("the generation Diffusion does not take nodata: set it on the super-resolution or SAR -> NDVI class")

    def sample(self, n, model, target_class=None, cfg_scale=3, input_channels=3, generate_video=False,
               noise_source=None, sampling_steps=None, eta=0.0):
        """Reference :206-259.  `sampling_steps` / `eta`: a DDIM chain, as in the super-resolution sampler."""
        return self._sample(n, model, target_class, cfg_scale, input_channels, generate_video, noise_source, sampling_steps,
                            eta)

    def sample_known(self, n, model, known, known_mask, target_class=None, cfg_scale=3, input_channels=3, resample=1, jump=1,
                     generate_video=False, noise_source=None, sampling_steps=None, eta=0.0):
        """Class-conditional inpainting: `sample` with known pixels, as in the super-resolution `sample_known` (the guidance
        is folded into the same update kernel)."""
        asks_for_known_pixels(known, known_mask, resample, jump, required=True)
        return self._sample(n, model, target_class, cfg_scale, input_channels, generate_video, noise_source, sampling_steps,
                            eta, known, known_mask, resample, jump)

    def sample_ensemble(self, n_members, model, target_class=None, cfg_scale=3, input_channels=3, member_batch=None,
                        sampling_steps=None, eta=0.0, noise_source=None, known=None, known_mask=None, resample=1, jump=1):
        """`n_members` >= 2 images per label of `target_class` (B labels; None: unconditional, B = 1), guided with
        `cfg_scale`: (n_members, B, C, S, S).  The super-resolution `sample_ensemble` - chunks of `member_batch` members, each
        one `sample` (with `known` / `known_mask`: `sample_known`) call on the labels repeated member-major."""
        labels = target_class.reshape(-1) if target_class is not None else None
        B = labels.numel() if labels is not None else 1
        args = {"cfg_scale": cfg_scale, "input_channels": input_channels, "noise_source": noise_source,
                "sampling_steps": sampling_steps, "eta": eta}

        def chunk(m):
            args["target_class"] = labels.repeat(m) if labels is not None else None
            return self._ensemble_chunk(m * B, (model,), _repeat_members(known, m), _repeat_members(known_mask, m), resample,
                                        jump, args)
        return self._sample_members(n_members, member_batch, B, chunk)

    def _sample(self, n, model, target_class, cfg_scale, input_channels, generate_video, noise_source, sampling_steps, eta,
                known=None, known_mask=None, resample=1, jump=1):
        check_sampling_args(self.noise_steps, sampling_steps, eta)
        check_inpaint_args((n, input_channels, self.image_size, self.image_size), known, known_mask, resample, jump)
        if target_class is not None:
            ncls = getattr(self._engine_net(model), "num_classes", None)
            if not target_class.is_cuda and ncls and target_class.numel() and int(target_class.max()) >= int(ncls):
                raise IndexError(f"target_class {int(target_class.max())} out of range for num_classes={ncls}")
            target_class = target_class.to(self.device)
        if cfg_scale > 0 and target_class is not None:
            # conditional and unconditional predictions as ONE 2n batch (label -1 = no embedding for that row) and
            # torch.lerp folded into the update kernel: half the launches of the reference's two forwards (:236-239)
            labels2 = torch.cat([target_class.to(torch.int64).expand(n) if target_class.numel() == 1
                                 else target_class.to(torch.int64), torch.full((n,), -1, dtype=torch.int64,
                                                                               device=target_class.device)]).contiguous()

            def predict(engine, x, t, first):
                eps2 = engine.forward(x.repeat(2, 1, 1, 1), t, None, 1, labels=labels2, check_weights=first)
                return eps2[:n], eps2[n:]
        else:
            def predict(engine, x, t, first):
                # cfg_scale > 0 without a class: lerp(u, u, w) == u, one forward is enough
                return engine.forward(x, t[:n], None, 1, labels=target_class, check_weights=first)
        # (row i of the 2n-wide timestep table: step i; the unguided forward takes n of the 2n)
        return self._sample_chain(model, (n, input_channels, self.image_size, self.image_size), predict, table_rows=2 * n,
                                  generate_video=generate_video, noise_source=noise_source, sampling_steps=sampling_steps,
                                  eta=eta, cfg_scale=cfg_scale, known=known, known_mask=known_mask, resample=resample,
                                  jump=jump)


class SyntheticClassDataset(torch.utils.data.Dataset):
    """Seeded (img, label) pairs shaped like torchvision ImageFolder items (reference :584-586 uses
    `train_loader.dataset.classes`)."""

    def __init__(self, length, channels, image_size, num_classes=10, seed=0):
        from .. import synthetic
        self.img = synthetic.tensor_uniform("synthetic.img", (length, channels, image_size, image_size), seed)
        self.label = synthetic.tensor_randint("synthetic.label", (length,), 0, num_classes, seed)
        self.classes = [str(i) for i in range(num_classes)]

    def __len__(self):
        return self.img.shape[0]

    def __getitem__(self, i):
        return self.img[i], self.label[i]


def class_folder_feed(args, device, rank=0, world_size=1):
    """The device feed of the class-folder tree `--dataset_path` (reference :573-584: ImageFolder + Resize((S, S)) + ToTensor; the
    path is used as given, the reference's `../` prefix belongs to its working directory).  With --scene_size P the images are
    decoded at P x P and the items are --image_size windows (augment.py)."""
    from ..augment import feed_kwargs, scene_size
    from ..feeds import DeviceClassFeed, load_class_folder_u8
    if not os.path.isdir(args.dataset_path):
        raise FileNotFoundError(f"--dataset_path {args.dataset_path!r}: expected a folder with one sub-folder of images per "
                                "class (or synthetic[:N[:classes]])")
    u8, labels, classes = load_class_folder_u8(args.dataset_path, scene_size(args), rank, world_size)
    if u8.shape[1] != args.inp_out_channels:
        raise ValueError(f"the images of {args.dataset_path} have {u8.shape[1]} bands, --inp_out_channels is {args.inp_out_channels}")
    return DeviceClassFeed(u8.to(device), labels.to(device), classes, args.batch_size, shuffle=True, **feed_kwargs(args, rank))


def launch(args):
    """Reference launch (:505-636).  `--dataset_path` is the reference's class-folder tree (decoded once with Pillow into a uint8
    cache on the device, batches gathered there; no validation set, as in the reference) or `synthetic[:N[:classes]]` (seeded
    images)."""
    if args.UNet_type.lower() != "residual attention unet":
        raise ValueError("The UNet type must be Residual Attention UNet")
    spec = str(args.dataset_path or "")
    if spec.lower() == "cifar10":
        raise ValueError("--dataset_path cifar10: the reference downloads CIFAR-10 through torchvision, which is not available "
                         "here; unpack the images into one folder per class and pass that folder")
    device = launch_device(args)
    ch = args.inp_out_channels
    if not spec.startswith("synthetic"):
        r, wsz = (drs_dist.rank(), drs_dist.world_size()) if args.multiple_gpus else (0, 1)
        train_loader, val_loader = class_folder_feed(args, device, r, wsz), None  # (reference :581-584, :625: val_loader=None)
    else:
        parts = spec.split(":")
        length = int(parts[1]) if len(parts) > 1 else 4 * args.batch_size
        ncls = int(parts[2]) if len(parts) > 2 else 10
        train_dataset = SyntheticClassDataset(length, ch, args.image_size, ncls, seed=1)
        val_dataset = SyntheticClassDataset(max(length // 4, 1), ch, args.image_size, ncls, seed=2)
        train_loader, val_loader = make_loaders(args, train_dataset, val_dataset)
        r = 0
    num_classes = len(train_loader.dataset.classes)
    model = Residual_Attention_UNet_generation(ch, ch, num_classes, device).to(device)
    diffusion = train_model(args, Diffusion, model, device, train_loader, val_loader)
    if r != 0:
        return  # a folder run on several ranks: one rank samples and writes the results

    def sample(i, **ddim):
        return diffusion.sample(n=5, model=model, target_class=torch.full((5,), i, dtype=torch.int64), cfg_scale=3,
                                input_channels=ch, generate_video=False, **ddim)
    save_final_samples(args, sample, range(min(num_classes, 3)), "generation_results.pt")


def build_arg_parser():
    """`base_arg_parser` and the generation flag of the reference (:649-665)."""
    p = base_arg_parser()
    p.add_argument("--inp_out_channels", type=int, default=3)
    return p


def train_main_parser():
    """`build_arg_parser`, the crop / augmentation flags (augment.add_augment_args) and the optimizer / resume and objective
    flags (cli.add_train_args): what `main` parses."""
    p = build_arg_parser()
    add_augment_args(p)
    return add_finetune_args(add_prediction_args(add_train_args(p), in_help=False))


def main(argv=None):
    parser = train_main_parser()
    args = check_train_args(parser, parser.parse_args(argv))
    args.snapshot_folder_path = os.path.join(os.curdir, "models_run", args.model_name, "weights")
    launch(args)


if __name__ == "__main__":
    main()
