"""Colour correction without a GPU: the float64 oracle of tests/colorfix_oracle.py against the definition, the C-ABI's argument
errors, `color_fix`'s ValueErrors and the command-line flags."""
import ctypes as C

import pytest
import torch

import colorfix_oracle as CO


def test_oracle_blur_is_the_index_clamp_definition():
    """F.pad(replicate) + dilated conv2d equals sum k_i k_j x[clamp(y + i d)][clamp(x + j d)] on a 5 x 7 plane, also for
    dilations beyond the plane, where both borders clamp at once."""
    g = torch.Generator().manual_seed(5)
    x = torch.rand((1, 2, 5, 7), generator=g, dtype=torch.float64)
    for d in (1, 2, 4, 8, 16):
        got = CO.blur(x, d)
        for c in range(2):
            want = CO.blur_by_index(x[0, c], d)
            assert (got[0, c] - want).abs().max().item() <= 4e-16, d
    # the weights sum to 1 and the decomposition telescopes
    assert (CO.blur(torch.full((1, 1, 5, 7), 0.3, dtype=torch.float64), 4) - 0.3).abs().max().item() <= 1e-16
    high, low = CO.decompose(x, 5)
    assert (high + low - x).abs().max().item() <= 1e-15


def test_one_pixel_image_returns_the_guide():
    """On a 1 x 1 image every tap clamps to the one pixel: low(x) = x, so the wavelet result is the guide, for every level
    count; so does a level whose dilation exceeds the plane return the plane's clamped taps only."""
    sr, guide = torch.tensor([[[[0.7]]]]), torch.tensor([[[[0.2]]]])
    for levels in (1, 3, 5):
        assert (CO.wavelet(sr, guide, levels) - guide.double()).abs().max().item() <= 4e-16
    same = torch.rand((1, 3, 5, 7), generator=torch.Generator().manual_seed(1))
    assert (CO.wavelet(same, same, 5) - same.double()).abs().max().item() <= 1e-15


def test_oracle_adain_moves_mean_and_deviation():
    g = torch.Generator().manual_seed(2)
    sr = 0.95 + 0.002 * torch.randn((2, 3, 9, 11), generator=g)
    guide = 0.4 + 0.1 * torch.randn((2, 3, 9, 11), generator=g)
    out = CO.adain(sr, guide)
    a, b = CO.adain_coefficients(sr, guide)
    assert (out - (a * sr.double() + b)).abs().max().item() <= 1e-12
    assert (out.mean(dim=(2, 3)) - guide.double().mean(dim=(2, 3))).abs().max().item() <= 1e-12
    want_std = torch.sqrt(guide.double().var(dim=(2, 3)) + 1e-5) * torch.sqrt(sr.double().var(dim=(2, 3)) / (sr.double().var(dim=(2, 3)) + 1e-5))
    assert (out.std(dim=(2, 3)) - want_std).abs().max().item() <= 1e-12


def test_argument_validation_without_gpu():
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    n = 3 * 16 * 16 * 4
    bufs = [C.create_string_buffer(n) for _ in range(3)]
    sr, guide, out = (C.cast(b, C.c_void_p) for b in bufs)
    ws_buf = C.create_string_buffer(1 << 16)
    ws = C.cast(ws_buf, C.c_void_p)

    def wavelet(ptrs=(sr, guide, out), shape=(1, 3, 16, 16), levels=5):
        return lib.drs_colorfix_wavelet(*ptrs, *shape, levels, None)

    def adain(ptrs=(sr, guide, out), shape=(1, 3, 16, 16), w=ws, w_bytes=1 << 16):
        return lib.drs_colorfix_adain(*ptrs, *shape, w, w_bytes, None)
    for fn in (wavelet, adain):
        for hole in range(3):
            assert fn(tuple(None if i == hole else p for i, p in enumerate((sr, guide, out)))) == 1
            assert b"null pointer" in lib.drs_last_error()
        # in place, and a window that starts inside an input
        assert fn((sr, guide, sr)) == 1 and b"overlaps" in lib.drs_last_error()
        assert fn((sr, guide, guide)) == 1 and b"overlaps" in lib.drs_last_error()
        assert fn((sr, guide, C.c_void_p(sr.value + n - 4))) == 1 and b"overlaps" in lib.drs_last_error()
        for shape in ((0, 3, 16, 16), (1, 0, 16, 16), (1, 3, 0, 16), (1, 3, 16, 0), (1, 17, 16, 16), (-1, 3, 16, 16)):
            assert fn(shape=shape) == 2, shape
    for levels in (0, 6, -1):
        assert wavelet(levels=levels) == 2 and b"levels" in lib.drs_last_error()
    assert adain(shape=(1, 3, 1, 1)) == 2 and b"variance" in lib.drs_last_error()
    assert adain(w=None) == 1 and b"null pointer" in lib.drs_last_error()
    assert adain(w_bytes=8) == 4
    need = lib.drs_colorfix_adain_workspace_bytes(1, 3, 16, 16)
    assert 0 < need <= 1 << 16 and adain(w_bytes=need - 1) == 4
    assert lib.drs_colorfix_adain_workspace_bytes(1, 17, 16, 16) == 0
    assert lib.drs_colorfix_adain_workspace_bytes(1, 3, 1, 1) == 0
    assert lib.drs_colorfix_adain_workspace_bytes(0, 3, 16, 16) == 0
    sizes = [lib.drs_colorfix_adain_workspace_bytes(b, 3, 40, 52) for b in (1, 2, 3, 16)]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4
    assert lib.drs_abi_version() == 8


def test_wrappers_have_no_cpu_path():
    from diffusionremotesensing_amd import color_fix, colorfix, hip_ops
    x = torch.rand(1, 3, 16, 16)
    for call in (lambda: hip_ops.colorfix_wavelet(x, x), lambda: hip_ops.colorfix_adain(x, x), lambda: color_fix(x, guide=x),
                 lambda: colorfix.color_fix(x, guide=x, method="adain"),
                 lambda: color_fix(x, x[:, :, :8, :8], magnification_factor=2)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


def test_color_fix_value_errors():
    from diffusionremotesensing_amd.colorfix import color_fix
    sr, lr = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 8, 8)
    with pytest.raises(ValueError, match="method"):
        color_fix(sr, guide=sr, method="histogram")
    with pytest.raises(ValueError, match="exactly one"):
        color_fix(sr, lr, guide=sr, magnification_factor=2)
    with pytest.raises(ValueError, match="exactly one"):
        color_fix(sr)
    with pytest.raises(ValueError, match="levels"):
        color_fix(sr, guide=sr, method="adain", levels=3)
    with pytest.raises(ValueError, match="levels"):
        color_fix(sr, guide=sr, method="adain", levels=5)
    for levels in (0, 6, 2.5, True):
        with pytest.raises(ValueError, match="levels"):
            color_fix(sr, guide=sr, levels=levels)
    with pytest.raises(ValueError, match="go together"):
        color_fix(sr, lr)
    with pytest.raises(ValueError, match="go together"):
        color_fix(sr, guide=sr, magnification_factor=2)
    with pytest.raises(ValueError, match="up-sampled"):
        color_fix(sr, lr, magnification_factor=4)
    with pytest.raises(ValueError, match="shape"):
        color_fix(sr, guide=sr[:, :, :8])
    with pytest.raises(ValueError, match="axes"):
        color_fix(sr[0], guide=sr)


def test_tiler_and_evaluate_refuse_bad_requests_before_sampling():
    """The checks run before anything touches the engine: a CPU tiler / Diffusion raises them."""
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    d = Diffusion("cosine", torch.nn.Identity(), "/nonexistent/snapshot.pt", noise_steps=8, device="cpu", magnification_factor=2,
                  image_size=16, Degradation_type="DownBlur")
    tiler = split_aggregation_sampling(torch.zeros(1, 3, 8, 12), 8, 4, 2, d, "cpu")
    for mode in ("final", "per_step"):
        with pytest.raises(ValueError, match="method"):
            tiler.aggregation_sampling(aggregation=mode, color_fix="histogram")
        with pytest.raises(ValueError, match="levels"):
            tiler.aggregation_sampling(aggregation=mode, color_fix="wavelet", color_fix_levels=6)
        with pytest.raises(ValueError, match="adain"):
            tiler.aggregation_sampling(aggregation=mode, color_fix="adain", color_fix_levels=3)
    loader = [(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 16, 16))]
    with pytest.raises(ValueError, match="method"):
        d.evaluate(d.model, loader, color_fix="histogram")
    with pytest.raises(ValueError, match="ensemble"):
        d.evaluate(d.model, loader, color_fix="wavelet", ensemble=4)
    with pytest.raises(ValueError, match="known_mask_fn"):
        d.evaluate(d.model, loader, color_fix="adain", known_mask_fn=lambda truth: torch.ones_like(truth[:, :1]))
    with pytest.raises(ValueError, match="levels"):
        d.evaluate(d.model, loader, color_fix="wavelet", color_fix_levels=0)


def test_flags_parse_on_both_command_lines():
    from diffusionremotesensing_amd import Aggregation_Sampling, colorfix, evaluate
    for p in (Aggregation_Sampling.build_arg_parser(), evaluate.cli_arg_parser("superres")):
        a = p.parse_args([])
        assert (a.color_fix, a.color_fix_levels) == ("none", 5) and colorfix.cli_color_fix(a) == {}
        a = p.parse_args(["--color_fix", "wavelet", "--color_fix_levels", "3"])
        assert colorfix.cli_color_fix(a) == {"color_fix": "wavelet", "color_fix_levels": 3}
        a = p.parse_args(["--color_fix", "adain"])
        assert colorfix.cli_color_fix(a) == {"color_fix": "adain", "color_fix_levels": 5}
        with pytest.raises(SystemExit):
            p.parse_args(["--color_fix", "histogram"])
    sar = evaluate.cli_arg_parser("sar_to_ndvi").parse_args([])
    assert not hasattr(sar, "color_fix") and colorfix.cli_color_fix(sar) == {}


def test_score_formatters_print_the_extra_row():
    from diffusionremotesensing_amd.evaluate import format_table
    from diffusionremotesensing_amd.train_diffusion_superres import format_scores
    row = {"psnr": 20.0, "ssim": 0.5, "sam": 3.0, "ergas": 12.0}
    plain = {"model": row, "bicubic": row}
    fixed = {"model": row, "bicubic": row, "model_fixed": dict(row, psnr=21.5)}
    assert "model_fixed" not in format_scores(plain) and "model_fixed" not in format_table(plain)
    assert " | model_fixed PSNR 21.50 dB " in format_scores(fixed)
    lines = format_table(fixed).splitlines()
    assert [ln.split()[0] for ln in lines[1:]] == ["model", "model_fixed", "bicubic"] and "21.50 dB" in lines[2]
    assert len({len(ln) for ln in lines}) == 1  # the columns stay aligned
    assert format_table(plain).splitlines()[1].startswith("model" + " " * 5)  # and the plain table is laid out as before
