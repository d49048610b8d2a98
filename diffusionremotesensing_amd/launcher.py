"""The pieces of a `launch` that the three trainers share: device and run directories, DataLoaders, the training run from the
flags, and the final sampling."""
import os

import torch

from . import cli
from . import dist as drs_dist


def launch_device(args):
    """The run directories and the device of a `launch`: RCCL process group + this rank's GPU with --multiple_gpus
    (reference :586-590), the visible one otherwise."""
    os.makedirs(args.snapshot_folder_path, exist_ok=True)
    os.makedirs(os.path.join(os.curdir, "models_run", args.model_name, "results"), exist_ok=True)
    if args.multiple_gpus:
        drs_dist.init_process_group()  # RCCL ("nccl" backend on ROCm), env:// rendezvous like reference :586
        gpu_id = int(os.environ["LOCAL_RANK"])
        torch.cuda.set_device(gpu_id)
        return gpu_id
    if not torch.cuda.is_available():
        raise RuntimeError("no ROCm device visible: this implementation has no CPU path")
    return torch.device("cuda")


def make_loaders(args, train_dataset, val_dataset):
    """(train, val) DataLoaders of a dataset pair: one shard per rank with --multiple_gpus, shuffled otherwise."""
    from torch.utils.data import DataLoader
    from torch.utils.data.distributed import DistributedSampler

    def loader(ds):
        if args.multiple_gpus:
            return DataLoader(ds, batch_size=args.batch_size, shuffle=False, sampler=DistributedSampler(ds))
        return DataLoader(ds, batch_size=args.batch_size, shuffle=True)
    return loader(train_dataset), loader(val_dataset)


def train_model(args, diffusion_class, model, device, train_loader, val_loader, train_kwargs=None, nodata=None,
                data_range=None, **diffusion_kwargs):
    """Same weights on every rank, `diffusion_class(...)` from the flags (a snapshot, if there is one, is loaded here),
    the training run, and the end of the process group.  `nodata`, `data_range`: the Diffusion's attributes of those names (None: left
    alone).  Returns the Diffusion."""
    print("Num params: ", sum(p.numel() for p in model.parameters()))
    if args.multiple_gpus:
        drs_dist.broadcast_module(model)  # what the DDP constructor does in the reference (:658)
    diffusion = diffusion_class(noise_schedule=args.noise_schedule, model=model,
                                snapshot_path=os.path.join(args.snapshot_folder_path, args.snapshot_name),
                                noise_steps=args.noise_steps, beta_start=1e-4, beta_end=0.02, device=device,
                                image_size=args.image_size, model_name=args.model_name, multiple_gpus=args.multiple_gpus,
                                ema_smoothing=args.ema_smoothing, **cli.cli_prediction(args), **cli.cli_threshold(args),
                                **cli.cli_ztsnr(args), **diffusion_kwargs)
    cli.set_guidance_rescale(diffusion, args)
    if nodata is not None:
        diffusion.nodata = nodata
    if data_range is not None:
        diffusion.data_range = data_range
    diffusion.train(lr=args.lr, epochs=args.epochs, check_preds_epoch=args.check_preds_epoch,
                    train_loader=train_loader, val_loader=val_loader, patience=args.patience, loss=args.loss,
                    verbose=True, **cli.train_kwargs(args), **cli.cli_finetune(args), **(train_kwargs or {}))
    if args.multiple_gpus:
        drs_dist.destroy_process_group()
    return diffusion


def save_final_samples(args, sample, conditions, file_name):
    """The final sampling of a `launch`: `sample(c, sampling_steps=, eta=)` for every c of `conditions` (the DDIM flags, or
    the ancestral chain), concatenated into models_run/<model_name>/results/<file_name>."""
    ddim = {"sampling_steps": getattr(args, "sampling_steps", None), "eta": getattr(args, "eta", 0.0)}
    outs = [sample(c, **ddim) for c in conditions]
    torch.save(torch.cat(outs).cpu(), os.path.join(os.getcwd(), "models_run", args.model_name, "results", file_name))
