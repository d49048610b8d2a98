"""Multispectral band counts on the host: the CPU oracle against the reference at 13 bands (tests/golden/
multispectral_golden.npz, tools/make_golden_multispectral.py), the `.npy` image folders of the superres data path, and the
band limit of drs_unet_plan_create (1 .. 16)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_errors

GOLDEN = "multispectral_golden.npz"
BANDS, SAR_BANDS, CLASSES = 13, 6, 10


@pytest.fixture(scope="module")
def msgolden():
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", GOLDEN))


def _sd(model):
    from diffusionremotesensing_amd import synthetic
    return synthetic.seeded_state_dict(model.state_dict(), 0)


def test_oracle_superres_13_bands(msgolden):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from oracle import unet_oracle as U
    sd = _sd(Residual_Attention_UNet_superres(BANDS, BANDS, "cpu"))
    x = synthetic.tensor_normal("ms.sr.x", (2, BANDS, 64, 64))
    lr = synthetic.tensor_uniform("ms.sr.lr", (2, BANDS, 32, 32))
    t = synthetic.tensor_randint("ms.sr.t", (2,), 1, 1500)
    with torch.no_grad():
        got = U.unet_forward(sd, x, t, lr, 2)
    assert max(rel_errors(got, torch.from_numpy(msgolden["ms_sr_out"]))) < 1e-5


def test_oracle_sar_6_bands(msgolden):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    from oracle import unet_oracle as U
    sd = _sd(Residual_Attention_UNet_SAR_TO_NDVI(SAR_BANDS, 1, "cpu"))
    x = synthetic.tensor_normal("ms.sar.x", (2, 1, 64, 64))
    sar = synthetic.tensor_uniform("ms.sar.sar", (2, SAR_BANDS, 64, 64))
    t = synthetic.tensor_randint("ms.sar.t", (2,), 1, 1500)
    with torch.no_grad():
        got = U.unet_forward_sar(sd, x, t, sar)
    assert max(rel_errors(got, torch.from_numpy(msgolden["ms_sar_out"]))) < 1e-5


def test_oracle_generation_13_bands(msgolden):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    from oracle import unet_oracle as U
    sd = _sd(Residual_Attention_UNet_generation(BANDS, BANDS, CLASSES, "cpu"))
    x = synthetic.tensor_normal("ms.gen.x", (2, BANDS, 32, 32))
    t = synthetic.tensor_randint("ms.gen.t", (2,), 1, 1500)
    with torch.no_grad():
        got = U.unet_forward_generation(sd, x, t, torch.tensor([3, 7]))
    assert max(rel_errors(got, torch.from_numpy(msgolden["ms_gen_out"]))) < 1e-5


def test_golden_chain_shape(msgolden):
    x = msgolden["ms_chain_x"]
    assert x.shape == (2, BANDS, 32, 32) and np.isfinite(x).all()


# ---- .npy image folders (degradation.load_image_folder_u8) ----

def _write(folder, name, arr):
    folder.mkdir(exist_ok=True)
    np.save(folder / name, arr)


def test_npy_folder_uint8_conversion(tmp_path):
    from diffusionremotesensing_amd.degradation import load_image_folder_u8
    rng = np.random.default_rng(1)
    ys = [rng.random((24, 20, BANDS)).astype(np.float32) for _ in range(3)]
    ys[0][0, 0, :] = [0.0, 1.0, 0.5, 0.999, 0.001, 0.25, 0.75, 1 / 255, 2 / 255, 0.3, 0.6, 0.9, 0.1]
    for i, y in enumerate(ys):
        _write(tmp_path / "d", f"img{i}.npy", y)
    u8 = load_image_folder_u8(str(tmp_path / "d"))
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (3, BANDS, 24, 20)
    for i, y in enumerate(ys):  # the reference's numpy data format: (y * 255).astype(np.uint8), bands first
        assert np.array_equal(u8[i].numpy(), np.moveaxis((y * 255).astype(np.uint8), -1, 0))


def test_npy_folder_resize_is_per_band_pillow_L(tmp_path):
    from PIL import Image

    from diffusionremotesensing_amd.degradation import load_image_folder_u8
    rng = np.random.default_rng(2)
    y = rng.random((37, 29, BANDS)).astype(np.float32)
    _write(tmp_path / "d", "a.npy", y)
    got = load_image_folder_u8(str(tmp_path / "d"), image_size=64)[0].numpy()
    u8 = (y * 255).astype(np.uint8)
    for b in range(BANDS):
        want = np.asarray(Image.fromarray(np.ascontiguousarray(u8[:, :, b])).resize((64, 64), Image.BILINEAR))
        assert np.array_equal(got[b], want), b


def test_npy_folder_three_bands_match_pillow_rgb(tmp_path):
    """At C = 3 the per-band L resize gives the bytes of Pillow's RGB resize of the same uint8 array."""
    from PIL import Image

    from diffusionremotesensing_amd.degradation import load_image_folder_u8
    rng = np.random.default_rng(3)
    y = rng.random((41, 33, 3)).astype(np.float32)
    _write(tmp_path / "d", "a.npy", y)
    for size in (64, 16):
        got = load_image_folder_u8(str(tmp_path / "d"), image_size=size)[0].numpy()
        rgb = Image.fromarray((y * 255).astype(np.uint8)).resize((size, size), Image.BILINEAR)
        assert np.array_equal(got, np.moveaxis(np.asarray(rgb), -1, 0)), size


def test_npy_folder_mixed_band_counts_raise(tmp_path):
    from diffusionremotesensing_amd.degradation import load_image_folder_u8
    _write(tmp_path / "d", "a.npy", np.zeros((16, 16, BANDS), np.float32))
    _write(tmp_path / "d", "b.npy", np.zeros((16, 16, 4), np.float32))
    with pytest.raises(ValueError, match="band count"):
        load_image_folder_u8(str(tmp_path / "d"), image_size=16)


def test_npy_folder_rejects_17_bands(tmp_path):
    from diffusionremotesensing_amd.degradation import load_image_folder_u8
    _write(tmp_path / "d", "a.npy", np.zeros((16, 16, 17), np.float32))
    with pytest.raises(ValueError, match="16"):
        load_image_folder_u8(str(tmp_path / "d"))


# ---- the band limit of the C-ABI ----

def _plan_create(cfg):
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    rc = lib.drs_unet_plan_create(C.byref(h), C.byref(cfg))
    if rc == 0:
        lib.drs_unet_plan_destroy(h)
    return rc, lib.drs_last_error()


@pytest.mark.parametrize("train", [0, 1], ids=["eval", "train"])
def test_plan_create_accepts_up_to_16_bands(train):
    from diffusionremotesensing_amd import _lib
    flags = _lib.PLAN_TRAIN if train else 0
    for impl in range(len(_lib.IMPL_BY_NAME)):
        for c in (1, 5, 13, 16):
            for cfg in (_lib.UNetConfig(2, 2, c, c, 64, 64, 2, impl, 1e-5, flags),
                        _lib.UNetConfig(2, 2, 1, 1, 64, 64, 1, impl, 1e-5, flags, _lib.VARIANT_SAR_TO_NDVI, c, 0),
                        _lib.UNetConfig(2, 2, c, c, 64, 64, 1, impl, 1e-5, flags, _lib.VARIANT_GENERATION, 0, 10)):
                rc, err = _plan_create(cfg)
                assert rc == 0, (impl, c, err)


def test_plan_create_rejects_17_bands_naming_16():
    from diffusionremotesensing_amd import _lib
    for cfg in (_lib.UNetConfig(2, 2, 17, 17, 64, 64, 2, 0, 1e-5, 0),
                _lib.UNetConfig(2, 2, 3, 17, 64, 64, 2, 0, 1e-5, 0),
                _lib.UNetConfig(2, 2, 17, 17, 64, 64, 1, 0, 1e-5, 0, _lib.VARIANT_GENERATION, 0, 10),
                _lib.UNetConfig(2, 2, 1, 1, 64, 64, 1, 0, 1e-5, 0, _lib.VARIANT_SAR_TO_NDVI, 17, 0)):
        rc, err = _plan_create(cfg)
        assert rc == 2, rc  # DRS_ERR_SHAPE
        assert b"16" in err and b"17" in err, err
