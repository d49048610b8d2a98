"""Per-step tile aggregation on the GPU: drs_gather_tiles and drs_blend_step / drs_blend_step_ddim against slicing and the
float64 step, `split_aggregation_sampling.sample_scene` against the layouts where it must reduce to the existing samplers,
and whole joint chains against the float64 oracle of tests/tile_chain_oracle.py."""
import pytest
import torch

import ddim_oracle as O
import tile_chain_oracle as TC
from conftest import replay_noise_source, replay_tile_noise
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
_ORACLE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _model(dev, sd, impl):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    return m


def _diffusion(m, dev, T, image_size=64):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                     image_size=image_size, Degradation_type="DownBlur")


def _randn(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# (LR height, LR width, patch, stride, magnification, channels): the three geometries of test_aggregate_tiles_kernel, one
# with odd x origins on a scene whose rows are 16-byte multiples (x0 = 5, magnification 1) and one whose rows are not
GEOMETRIES = ((48, 56, 32, 16, 2, 3), (20, 20, 8, 8, 1, 1), (24, 40, 16, 12, 2, 5), (16, 20, 8, 5, 1, 2), (20, 21, 8, 8, 1, 3))


# ---------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------
def test_gather_tiles_kernel(dev):
    """drs_gather_tiles is a copy: bit-equal to slicing, whole set and in chunks (the last one padded with repeats)."""
    from diffusionremotesensing_amd import hip_ops
    odd = False
    for (h, w, ps, st, m, C) in GEOMETRIES:
        infos, _ = A.tile_infos(h, w, ps, st, m)
        S, Hs, Ws = ps * m, h * m, w * m
        odd = odd or any(i[2] % 2 for i in infos)
        scene = _randn(h * 100 + w, (C, Hs, Ws))
        want = TC.gather(scene, infos)
        org = hip_ops.tile_origins([(i[0], i[2]) for i in infos], S, Hs, Ws, dev)
        got = hip_ops.gather_tiles(scene.to(dev), org, S)
        assert got.shape == want.shape and torch.equal(got.cpu(), want), (h, w)
        n, chunk = len(infos), 4
        out = torch.full((chunk, C, S, S), float("nan"), device=dev)
        for c0 in range(0, n, chunk):
            hip_ops.gather_tiles(scene.to(dev), org, S, out=out, first=c0, count=chunk)
            idx = [min(c0 + k, n - 1) for k in range(chunk)]
            assert torch.equal(out.cpu(), want[idx]), (h, w, c0)
    assert odd
    with pytest.raises(RuntimeError, match="elements"):
        hip_ops.gather_tiles(scene.to(dev), org, S, out=torch.empty((1, C, S, S), device=dev), count=2)


def _ancestral_coefficients(t, alpha, alpha_hat, beta):
    a, ah, b = float(alpha[t]), float(alpha_hat[t]), float(beta[t])
    return 1 / a ** 0.5, (1 / a ** 0.5) * (1 - a) / (1 - ah) ** 0.5, b ** 0.5


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_blend_step_kernel_vs_float64_oracle(dev, kind):
    """drs_blend_step / drs_blend_step_ddim against the float64 weighted mean + float64 step, eps of amplitude ~1:
    error / max(|A x| + |B eps| + |sigma z|) <= 1e-6 (the bound of drs_ddim_step, which measures 1.3e-7), bit-stable over
    calls.  Measured on MI355X: worst 1.5e-7 (linear) / 1.3e-7 (cosine), over layouts with up to 6 covering tiles per pixel: the
    fp32 weighted mean does not show next to the step's own rounding, and the bound is not widened."""
    from diffusionremotesensing_amd import hip_ops
    T = 1500
    alpha, ah, beta = D.schedule(kind, T)
    a_d, ah_d, b_d = alpha.to(dev), ah.to(dev), beta.to(dev)
    worst = 0.0
    layouts = GEOMETRIES[:1] + ((16, 24, 8, 8, 2, 3), (8, 8, 8, 8, 2, 3)) + GEOMETRIES[2:]  # overlap, partition, one tile, ...
    for (h, w, ps, st, m, C) in layouts:
        infos, _ = A.tile_infos(h, w, ps, st, m)
        S, Hs, Ws = ps * m, h * m, w * m
        wt = A.gaussian_weight(S, S)
        x, z = _randn(1, (1, C, Hs, Ws)), _randn(2, (1, C, Hs, Ws))
        eps_tiles = _randn(3, (len(infos), C, S, S))
        eps64 = TC.blend(eps_tiles, infos, wt, Hs, Ws)[None]
        org = hip_ops.tile_origins([(i[0], i[2]) for i in infos], S, Hs, Ws, dev)
        xd, zd, ed, wd = x.to(dev), z.to(dev), eps_tiles.to(dev), wt.to(dev)
        cases = [(t, None, 0.0) for t in (1499, 700, 2, 1)]
        cases += [(t, tp, eta) for (t, tp) in ((49, 42), (1499, 1469), (7, 1), (1, 0), (1499, 0)) for eta in (0.0, 0.5, 1.0)]
        for t, tp, eta in cases:
            if tp is None:
                cA, cB, sigma = _ancestral_coefficients(t, alpha, ah, beta)
                noise = z if t > 1 else None
                if noise is None:
                    sigma = 0.0
            else:
                cA, cB, sigma = O.coefficients(t, tp, eta, ah)
                noise = z if eta > 0 else None
            want = TC.step(x, eps64, noise, t, tp, eta, alpha, ah, beta)
            scale = (cA * x.double()).abs() + (cB * eps64).abs()
            if sigma > 0:
                scale = scale + (sigma * z.double()).abs()
            outs = []
            for _ in range(2):
                unc = torch.zeros(1, dtype=torch.int32, device=dev)
                s = xd[0].clone()
                hip_ops.blend_step_(s, ed, org, wd, zd[0] if noise is not None else None, t, alpha_hat=ah_d, alpha=a_d,
                                    beta=b_d, t_prev=tp, eta=eta, uncovered=unc)
                assert int(unc.item()) == 0
                outs.append(s.cpu())
            assert torch.equal(outs[0], outs[1]), (h, w, t, tp, eta)
            err = ((outs[0].double() - want[0]).abs().max() / scale.max()).item()
            worst = max(worst, err)
            assert err <= 1e-6, (kind, (h, w, ps, st, m, C), t, tp, eta, err, cA, cB, sigma)
    print(f"blend step kernel [{kind}]: worst normalised error {worst:.3e}")


def test_blend_step_counts_uncovered_pixels_and_rejects_bad_tensors(dev):
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 50)
    ah_d = ah.to(dev)
    S = 8
    scene = torch.zeros((1, 8, 16), device=dev)
    eps = torch.zeros((1, 1, S, S), device=dev)
    wt = A.gaussian_weight(S, S).to(dev)
    org = hip_ops.tile_origins([(0, 0)], S, 8, 16, dev)
    unc = torch.zeros(1, dtype=torch.int32, device=dev)
    hip_ops.blend_step_(scene, eps, org, wt, None, 10, alpha_hat=ah_d, t_prev=5, uncovered=unc)
    hip_ops.blend_step_(scene, eps, org, wt, None, 5, alpha_hat=ah_d, t_prev=0, uncovered=unc)
    assert int(unc.item()) == 2 * 8 * 8  # the right half of the scene, counted by both calls (the counter is not reset)
    assert torch.isfinite(scene[:, :, :8]).all()
    with pytest.raises(RuntimeError, match="noise"):
        hip_ops.blend_step_(scene, eps, org, wt, None, 10, alpha_hat=ah_d, t_prev=5, eta=0.5)
    with pytest.raises(RuntimeError, match="eps_tiles"):
        hip_ops.blend_step_(scene, torch.zeros((1, 2, S, S), device=dev), org, wt, None, 10, alpha_hat=ah_d, t_prev=5)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.blend_step_(scene, eps, org, wt, None, 10, alpha_hat=ah, t_prev=5)  # the table must live on the device


# ---------------------------------------------------------------------------------------------
# layouts where the joint chain is an existing sampler
# ---------------------------------------------------------------------------------------------
# One blended eps of a pixel one tile covers is (w * e) / w: two roundings, at most 1 ulp away from e, where the per-tile
# samplers use e itself; the step arithmetic is shared.  The bound allows that ulp a gain of 8 through the UNet forwards of
# the remaining steps: 8 ulp of the largest state per step.  Measured on MI355X (T = 8, mfma_f32, ancestral / DDIM S = 5
# eta 1): one tile 0.45 / 0.47 ulp per step, partition 0.34 / 0.36 ulp per step.
ULPS_PER_STEP = 8


def _assert_ulps_per_step(got, want, steps, what):
    err = (got.double() - want.double()).abs().max().item()
    per_step = err / (ULP * want.abs().max().item()) / steps
    print(f"{what}: max abs difference {err:.3e} = {per_step:.2f} ulp of max |x| per step over {steps} steps")
    assert torch.isfinite(got).all()
    assert per_step <= ULPS_PER_STEP, (what, err, per_step)


@pytest.mark.parametrize("S_eta", [(None, 0.0), (5, 1.0)])
def test_one_tile_scene_agrees_with_diffusion_sample(dev, seeded_sd, S_eta):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    S, eta = S_eta
    T = 8
    m = _model(dev, seeded_sd, "mfma_f32")
    d = _diffusion(m, dev, T)
    img = synthetic.tensor_uniform("tilechain.one", (1, 3, 32, 32)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 32, 2, d, dev)
    assert len(tiler.patches_lr) == 1
    got = tiler.sample_scene(noise_source=replay_noise_source(77), sampling_steps=S, eta=eta).cpu()
    assert m.training  # the samplers' side effect
    m.eval()
    want = d.sample(1, m, img[0], input_channels=3, noise_source=replay_noise_source(77), sampling_steps=S, eta=eta).cpu()
    assert got.shape == (3, 64, 64)
    _assert_ulps_per_step(got, want[0], T - 1 if S is None else S, f"one tile S={S}")


@pytest.mark.parametrize("S_eta", [(None, 0.0), (5, 1.0)])
def test_partition_layout_agrees_with_stitched_sample_tiles(dev, seeded_sd, S_eta):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    S, eta = S_eta
    T = 8
    m = _model(dev, seeded_sd, "mfma_f32")
    d = _diffusion(m, dev, T)
    img = synthetic.tensor_uniform("tilechain.part", (1, 3, 32, 64)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 32, 2, d, dev)
    infos = tiler.patches_sr_infos
    assert infos == [(0, 64, 0, 64), (0, 64, 64, 128)]
    shape = (1, 3, 64, 128)
    draws = {}

    def scene_src(i, shp):
        assert tuple(shp) == shape
        if i not in draws:
            draws[i] = _randn(9000 + i, shape)
        return draws[i]

    def tile_src(k, i, shp):
        y0, y1, x0, x1 = infos[k]
        return scene_src(i, shape)[:, :, y0:y1, x0:x1]
    got = tiler.sample_scene(noise_source=scene_src, sampling_steps=S, eta=eta).cpu()
    m.eval()
    tiles = tiler.sample_tiles(noise_source=tile_src, sampling_steps=S, eta=eta).cpu()
    want = torch.cat([tiles[0], tiles[1]], dim=2)
    _assert_ulps_per_step(got, want, T - 1 if S is None else S, f"partition S={S}")


# ---------------------------------------------------------------------------------------------
# whole joint chains against the float64 oracle
# ---------------------------------------------------------------------------------------------
# Max-abs error of the un-clamped scene against the float64 oracle chain, per chain (T, S, eta): (exact fp32, split bf16),
# ~10x the error measured on MI355X (the same for both tile_batch settings):
#   ancestral T = 8             2.1e-5 / 3.3e-4   on a state of max |x| =  42
#   DDIM T = 50, S = 10, eta 0  2.8e-4 / 4.7e-3   on a state of max |x| = 223
#   DDIM T = 50, S = 10, eta 1  7.2e-4 / 2.3e-2   on a state of max |x| = 307
# Above the final mode's bars at this shape (3e-5 / 5e-4) because those compare images clamped to [0, 1], where 95 - 99% of
# these pixels saturate, and this compares the raw state the untrained weights drive to 42 - 307: relative to max |x| the
# errors are 5e-7 - 2.3e-6 (exact fp32) and 8e-6 - 7.5e-5 (split bf16), those of the per-tile chains of test_gpu_ddim.py.
CHAIN_BOUNDS = {(8, None, 0.0): (2e-4, 3.5e-3), (50, 10, 0.0): (3e-3, 5e-2), (50, 10, 1.0): (7e-3, 2.5e-1)}
CHAINS = [(8, None, 0.0), (50, 10, 0.0), (50, 10, 1.0)]


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
@pytest.mark.parametrize("T,S,eta", CHAINS)
def test_joint_chain_vs_float64_oracle(dev, seeded_sd, impl, T, S, eta):
    """The scene of the tiler's golden test (LR 48x56, patch 32, stride 16, x2: 6 overlapping tiles of 64x64) through
    `sample_scene`, un-clamped (random weights push most pixels outside [0, 1]), with tile_batch = 16 (one chunk,
    conditioning reused) and 4 (two chunks, the last one padded, conditioning recomputed), against the float64 oracle chain
    over the fp32 oracle UNet.  The two settings agree to the bit on the exact-fp32 kernels."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    m = _model(dev, seeded_sd, impl)
    d = _diffusion(m, dev, T)
    img = synthetic.tensor_uniform("g10.img", (1, 3, 48, 56))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(48, 56, 32, 16, 2)
    assert [tuple(i) for i in tiler.patches_sr_infos] == infos and len(infos) == 6
    seed = 4000 + T + (S or 0) + int(10 * eta)

    def oracle():
        lr_tiles = torch.stack([img[0, :, y0:y0 + 32, x0:x0 + 32] for (y0, x0) in lr_origins])
        return TC.chain(TC.unet_eps_fn(U.OracleUNet(seeded_sd), lr_tiles, 2), 3, 96, 112, infos, A.gaussian_weight(64, 64), T,
                        D.schedule("cosine", T), replay_noise_source(seed), S, eta)
    key = (T, S, eta)
    if key not in _ORACLE:
        _ORACLE[key] = oracle()
    want = _ORACLE[key]
    outs = {}
    for tile_batch in (16, 4):
        tiler.tile_batch = tile_batch
        got = tiler.sample_scene(noise_source=replay_noise_source(seed), sampling_steps=S, eta=eta).cpu()
        m.eval()
        assert got.shape == (3, 96, 112) and torch.isfinite(got).all()
        err = (got.double() - want).abs().max().item()
        outside = ((want < 0) | (want > 1)).double().mean().item()
        top = want.abs().max().item()
        print(f"joint chain T={T} S={S} eta={eta} [{impl}] tile_batch={tile_batch}: max abs error {err:.3e} = {err / top:.2e} "
              f"of max |x| {top:.2f} ({100 * outside:.0f}% of the pixels outside [0, 1])")
        assert err <= CHAIN_BOUNDS[(T, S, eta)][impl == "mfma_bf16x3"], (impl, T, S, eta, tile_batch, err)
        outs[tile_batch] = got
    if impl == "mfma_f32":
        assert torch.equal(outs[16], outs[4])  # same kernels, same summation order, whatever the chunking


def test_per_step_mode_clamps_broadcasts_and_draws_like_the_samplers(dev, seeded_sd):
    """aggregation="per_step" is clamp(sample_scene) broadcast over img_lr's batch; an eta = 0 chain asks the noise source
    for x_T and nothing else."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T = 20
    m = _model(dev, seeded_sd, "mfma_f32")
    d = _diffusion(m, dev, T)
    img = synthetic.tensor_uniform("tilechain.batch", (2, 3, 32, 48)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)
    calls = []

    def src(i, shape):
        calls.append((i, tuple(shape)))
        return _randn(123 + i, shape)
    out = tiler.aggregation_sampling(noise_source=src, sampling_steps=4, eta=0.0, aggregation="per_step")
    assert calls == [(T, (1, 3, 64, 96))]
    m.eval()
    scene = tiler.sample_scene(noise_source=src, sampling_steps=4, eta=0.0)
    assert out.shape == (2, 3, 64, 96)
    assert torch.equal(out[0], scene.clamp(0, 1)) and torch.equal(out[0], out[1])
    assert out.min().item() >= 0 and out.max().item() <= 1


def test_final_mode_is_unchanged(dev, seeded_sd):
    """aggregation="final" is the default path: the same call with and without the argument returns the same bits."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T = 8
    m = _model(dev, seeded_sd, "mfma_f32")
    d = _diffusion(m, dev, T)
    img = synthetic.tensor_uniform("g10.img", (1, 3, 48, 56)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)
    src = replay_tile_noise(1010, len(tiler.patches_lr), T, (1, 3, 64, 64))
    a = tiler.aggregation_sampling(noise_source=src)
    m.eval()
    b = tiler.aggregation_sampling(noise_source=src, aggregation="final")
    assert torch.equal(a, b)
    m.eval()
    c = tiler.aggregation_sampling(noise_source=src, sampling_steps=5, eta=0.0)
    m.eval()
    e = tiler.aggregation_sampling(noise_source=src, sampling_steps=5, eta=0.0, aggregation="final")
    assert torch.equal(c, e)
