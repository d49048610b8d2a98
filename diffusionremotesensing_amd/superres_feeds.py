"""The data of a super-resolution run: `make_superres_feeds(args, device)` -> (train feed, validation feed, the LR images the
final sampling conditions on) for the reference's image folder or the seeded `synthetic[:N]` / `synthetic_u8[:N]` patches."""
import os

import torch

from . import dist as drs_dist
from .augment import centre_items, crop_d4_u8, feed_kwargs, scene_size, upload_items
from .bsr import DeviceBSRFeed
from .degradation import DeviceSuperresFeed, add_reference_noise, downblur, load_image_folder_u8
from .launcher import make_loaders


class SyntheticSuperresDataset(torch.utils.data.Dataset):
    """Seeded Gaussian/uniform (lr, hr) patches with the shapes `get_data_superres` yields (reference
    utils.py:93-166): the reference's image-folder datasets (PIL / torchvision) are outside the hot path and
    BASELINE.json's configs are all "synthetic"."""

    def __init__(self, length, channels, image_size, magnification_factor, seed=0):
        from . import synthetic
        s = image_size // magnification_factor
        self.hr = synthetic.tensor_uniform("synthetic.hr", (length, channels, image_size, image_size), seed)
        self.lr = synthetic.tensor_uniform("synthetic.lr", (length, channels, s, s), seed)

    def __len__(self):
        return self.hr.shape[0]

    def __getitem__(self, i):
        return self.lr[i], self.hr[i]


# -- the two device feeds -----------------------------------------------------------------------------------------------------
# Both builders return (make_feed(u8, fixed=False), first_items(u8, train_feed)): the feed of a uint8 HR cache for rank r, and the
# LR images of the final sampling from the first training images `u8`.  --scene_size P: the cache holds P x P scenes and every
# item is an --image_size window of one, cut on the device (augment.py); train feeds draw window and symmetry, validation feeds
# (`fixed`) and the final sampling take the centre window.

def _bsrgan_feed_makers(args, device, r):
    """The blind degradation, fresh for every batch on the device (bsr.py); rank r draws its own recipes; the validation feed
    starts from its seed at every epoch (the reference's frozen validation set)."""
    kind, seed = getattr(args, "bsr_kind", "plus"), getattr(args, "bsr_seed", 0)

    def make_feed(u8, fixed=False):
        return DeviceBSRFeed(u8.to(device), args.magnification_factor, args.batch_size, shuffle=not fixed, kind=kind,
                             seed=seed + (1 if fixed else 2 + r), fixed=fixed, **feed_kwargs(args, r, fixed))

    def first_items(u8, train_feed):  # the first training images under the fixed seed (the train feed has nothing to add)
        feed = DeviceBSRFeed(u8.to(device), args.magnification_factor, 1, shuffle=False, kind=kind, seed=seed, fixed=True,
                             **feed_kwargs(args, fixed=True))
        return [feed.item(i)[0] for i in range(u8.shape[0])]
    return make_feed, first_items


def _downblur_feed_makers(args, device, r):
    """The reference's DownBlur feed (utils.get_data_superres: bicubic down-sampling + Gaussian blur per item with Pillow on the
    host) from a uint8 HR cache on the device, bit-exact (degradation.py); DownBlurNoise adds its noise (reference :612-616:
    Gauss_noise=True)."""
    cache_size = scene_size(args)
    gauss_noise = args.Degradation_type.lower() == "downblurnoise"
    radius = args.Blur_radius if args.Blur_radius == "random" else float(args.Blur_radius)

    def make_feed(u8, fixed=False):
        return DeviceSuperresFeed(u8.to(device), args.magnification_factor, radius, args.batch_size, shuffle=True,
                                  Gauss_noise=gauss_noise, **feed_kwargs(args, r, fixed))

    def first_items(u8, train_feed):  # the first training images' centre windows, blurred with the radius the train feed drew
        if cache_size != args.image_size:
            items = centre_items(range(u8.shape[0]), cache_size, cache_size, args.image_size)
            u8 = crop_d4_u8(u8.to(device), upload_items(items, device), args.image_size)
        final_x = downblur(u8.to(device), args.magnification_factor, train_feed.blur_radius)[0]
        if gauss_noise:
            add_reference_noise(final_x, noise_level1=2, noise_level2=10)
        return [final_x[i] for i in range(final_x.shape[0])]
    return make_feed, first_items


def _mtf_feed_makers(args, device, r):
    """The sensor-MTF degradation (mtf.py): blur with each band's own Gaussian, decimate, optional noise, per batch on the device;
    rank r draws its own noise; the validation feed repeats its noise at every epoch."""
    from .mtf import DeviceMTFFeed

    def make_feed(u8, fixed=False):
        return DeviceMTFFeed(u8.to(device), args.magnification_factor, args.mtf_nyquist, getattr(args, "mtf_noise", None),
                             args.batch_size, shuffle=True, seed=1 if fixed else 2, fixed=fixed, **feed_kwargs(args, r, fixed))

    def first_items(u8, train_feed):  # the first training images' centre windows through the same operator, without noise
        feed = DeviceMTFFeed(u8.to(device), args.magnification_factor, args.mtf_nyquist, None, 1, shuffle=False, fixed=True,
                             **feed_kwargs(args, fixed=True))
        return [feed.item(i)[0] for i in range(u8.shape[0])]
    return make_feed, first_items


def _folder_feeds(args, device, spec, make_feed, first_items, r, wsz):
    """An image folder, laid out as the reference expects it (:597-598): <dataset_path>/train_original, /val_original.
    Decoded once with Pillow into the uint8 cache (this rank's shard only: rank r owns every world-th image like
    DistributedSampler); resize / blur / noise per batch on the device."""
    cache_size, ch = scene_size(args), args.inp_out_channels
    if not os.path.isdir(os.path.join(spec, "train_original")) or not os.path.isdir(os.path.join(spec, "val_original")):
        raise FileNotFoundError(f"--dataset_path {spec!r}: expected the folders train_original/ and val_original/ "
                                "(or synthetic[:N] / synthetic_u8[:N])")
    train_loader = make_feed(load_image_folder_u8(os.path.join(spec, "train_original"), cache_size, r, wsz))
    val_loader = make_feed(load_image_folder_u8(os.path.join(spec, "val_original"), cache_size, r, wsz), fixed=True)
    for what, feed in (("train_original", train_loader), ("val_original", val_loader)):
        if feed.hr.shape[1] != ch:
            raise ValueError(f"the images of {what} have {feed.hr.shape[1]} channels, --inp_out_channels is {ch}")
    # the final sampling conditions on train_dataset[0..4] of the WHOLE sorted folder (reference :678-680), whatever this
    # rank's shard holds; with Gauss_noise the dataset item carries its noise (utils.py:126-138)
    first = load_image_folder_u8(os.path.join(spec, "train_original"), cache_size, limit=5).to(device)
    return train_loader, val_loader, first_items(first, train_loader)


def _synthetic_feeds(args, device, spec, makers, r, wsz):
    """`synthetic[:N]`: seeded float (lr, hr) pairs through DataLoaders (`makers` None); `synthetic_u8[:N]`: the same HR patches
    as a uint8 cache through the device feed of `makers`."""
    ch = args.inp_out_channels
    length = int(spec.split(":")[1]) if ":" in spec else 4 * args.batch_size
    size = scene_size(args) if makers is not None else args.image_size  # (the float DataLoader path has no windows)
    train_dataset = SyntheticSuperresDataset(length, ch, size, args.magnification_factor, seed=1)
    val_dataset = SyntheticSuperresDataset(max(length // 4, 1), ch, size, args.magnification_factor, seed=2)
    final_lr = [train_dataset[i][0] for i in range(min(5, len(train_dataset)))]
    if makers is None:
        return (*make_loaders(args, train_dataset, val_dataset), final_lr)
    make_feed, first_items = makers

    def to_u8(hr):
        return (hr * 255).round().clamp(0, 255).to(torch.uint8)

    def feed(ds, fixed=False):
        # equal shard sizes on every rank (DistributedSampler pads; here the remainder is dropped): ranks must run
        # the same number of steps, or the per-step all-reduce of the longer shard never completes
        per_rank = len(ds) // wsz
        if per_rank == 0:
            raise ValueError(f"dataset of {len(ds)} images cannot be sharded over {wsz} ranks")
        return make_feed(to_u8(ds.hr[r::wsz][:per_rank]), fixed)
    train_loader, val_loader = feed(train_dataset), feed(val_dataset, fixed=True)
    if args.Degradation_type.lower() in ("bsrgan", "mtf") or size != args.image_size:
        # (a DownBlur run without windows conditions on the dataset's own seeded LR patches, like the float path)
        final_lr = first_items(to_u8(train_dataset.hr[:5]), train_loader)
    return train_loader, val_loader, final_lr


def _u16_feeds(args, device, spec, r, wsz):
    """--bit_depth 16 (radiometry.py): `<dataset_path>/train_original` and `/val_original` hold 16-bit files
    at the cache's size, or `synthetic_u16[:N]` - the `synthetic` HR patches as round(hr * 10000) -, kept as uint16 caches on the
    device and fed by `DeviceU16SuperresFeed`.  The band ranges are `args.data_range_table` (what `evaluate` read from the
    snapshot), else --data_range: given, or the percentiles of the training cache, summed over the ranks under --multiple_gpus.
    Both feeds carry the table as `data_range`."""
    from . import radiometry as R
    R.check_args(args)
    cache_size, ch = scene_size(args), args.inp_out_channels
    if spec.startswith("synthetic_u16"):
        length = int(spec.split(":")[1]) if ":" in spec else 4 * args.batch_size
        sets = [SyntheticSuperresDataset(n, ch, cache_size, args.magnification_factor, seed=s)
                for n, s in ((length, 1), (max(length // 4, 1), 2))]
        if min(len(ds) // wsz for ds in sets) == 0:
            raise ValueError(f"datasets of {[len(ds) for ds in sets]} images cannot be sharded over {wsz} ranks")
        train, val = (R.synthetic_u16(ds.hr[r::wsz][:len(ds) // wsz]) for ds in sets)
        first = R.synthetic_u16(sets[0].hr[:5])
    else:
        if not os.path.isdir(os.path.join(spec, "train_original")) or not os.path.isdir(os.path.join(spec, "val_original")):
            raise FileNotFoundError(f"--dataset_path {spec!r}: expected the folders train_original/ and val_original/ "
                                    "(or synthetic_u16[:N])")
        train = R.load_folder_u16(os.path.join(spec, "train_original"), cache_size, r, wsz)
        val = R.load_folder_u16(os.path.join(spec, "val_original"), cache_size, r, wsz)
        first = R.load_folder_u16(os.path.join(spec, "train_original"), cache_size, limit=5)
    for what, cache in (("train_original", train), ("val_original", val)):
        if cache.shape[1] != ch:
            raise ValueError(f"the images of {what} have {cache.shape[1]} channels, --inp_out_channels is {ch}")
    train, val, nodata = train.to(device), val.to(device), getattr(args, "nodata", None)
    table = getattr(args, "data_range_table", None)
    if table is None:
        table = R.resolve_range(getattr(args, "data_range", None), train, nodata, all_ranks=bool(args.multiple_gpus))
    table = R.check_table(table, ch)
    print(f"16-bit radiometry: band ranges {R.format_table(table)}")
    if args.Degradation_type.lower() == "mtf":  # the same caches under the sensor-MTF degradation (mtf.py)
        from .mtf import DeviceMTFFeed

        def make_mtf(cache, fixed=False, noise=getattr(args, "mtf_noise", None), batch=args.batch_size, rank=r):
            return DeviceMTFFeed(cache, args.magnification_factor, args.mtf_nyquist, noise, batch, shuffle=not fixed or batch > 1,
                                 data_range=table, nodata=nodata, seed=1 if fixed else 2, fixed=fixed,
                                 **feed_kwargs(args, rank, fixed))
        firsts = make_mtf(first.to(device), fixed=True, noise=None, batch=1, rank=0)
        return make_mtf(train), make_mtf(val, fixed=True), [firsts.item(i)[0] for i in range(first.shape[0])]
    radius = args.Blur_radius if args.Blur_radius == "random" else float(args.Blur_radius)

    def make_feed(cache, fixed=False):  # ("random": one draw per feed, as the 8-bit feeds)
        return R.DeviceU16SuperresFeed(cache, args.magnification_factor, radius, args.batch_size, True, table, nodata,
                                       **feed_kwargs(args, r, fixed))
    train_loader, val_loader = make_feed(train), make_feed(val, fixed=True)
    # the final sampling conditions on the first training images of the WHOLE list (centre windows), blurred as the train feed blurs
    firsts = R.DeviceU16SuperresFeed(first.to(device), args.magnification_factor, train_loader.blur_radius, 1, False, table, nodata,
                                     **feed_kwargs(args, fixed=True))
    return train_loader, val_loader, [firsts.item(i)[0] for i in range(first.shape[0])]


def make_superres_feeds(args, device):
    """(train feed, validation feed, the LR images the final sampling conditions on) of `--dataset_path`: the reference's
    image folder or `synthetic[:N]` / `synthetic_u8[:N]` (see `train_diffusion_superres.launch`); with --bit_depth 16 the uint16
    entrance (`_u16_feeds`)."""
    spec = str(args.dataset_path or "")
    r, wsz = (drs_dist.rank(), drs_dist.world_size()) if args.multiple_gpus else (0, 1)
    if int(getattr(args, "bit_depth", 8) or 8) == 16 or getattr(args, "data_range", None) is not None or \
            spec.startswith("synthetic_u16"):
        return _u16_feeds(args, device, spec, r, wsz)
    makers = None
    if not spec.startswith("synthetic") or spec.startswith("synthetic_u8"):
        kind = args.Degradation_type.lower()
        build = _bsrgan_feed_makers if kind == "bsrgan" else _mtf_feed_makers if kind == "mtf" else _downblur_feed_makers
        makers = build(args, device, r)
    if spec.startswith("synthetic"):
        return _synthetic_feeds(args, device, spec, makers, r, wsz)
    return _folder_feeds(args, device, spec, *makers, r, wsz)
