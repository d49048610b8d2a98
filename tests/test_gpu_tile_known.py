"""Known pixels in the tiler on the GPU: drs_blend_step_known and drs_aggregate_tiles_known against the kernels they extend
(bit for bit) and the float64 oracles, and `split_aggregation_sampling` with `known` / `known_mask` - super-resolution and
SAR -> NDVI scenes, both aggregation modes - against `sample_known` and the float64 joint chain of tests/tile_known_oracle.py."""
import pytest
import torch

import ddim_oracle as O
import inpaint_oracle as I
import tile_chain_oracle as TC
import tile_known_oracle as TK
from conftest import replay_noise_source
from oracle import aggregation_oracle as A
from oracle import diffusion_oracle as D
from oracle import unet_oracle as U
from test_gpu_tile_chain import CHAIN_BOUNDS, GEOMETRIES, ULPS_PER_STEP

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
MASK_SEED = 1  # tests/test_tile_known_host.py checks these block masks on the layouts below without a GPU
_ORACLE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _randn(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _sr_model(dev, sd, impl):
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    return m


def _sr_diffusion(m, dev, T):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    return Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=T, device=dev, magnification_factor=2,
                     image_size=64, Degradation_type="DownBlur")


def _sar_model(dev, sd, impl):
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    m = Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.hip_engine().set_impl(impl)
    return m


def _scene_mask(infos, Hs, Ws):
    """The seeded block mask of a scene: 30 - 70 % known, every tile holding known and unknown pixels."""
    mask = TK.block_mask(MASK_SEED, Hs, Ws)
    TK.check_mask(mask, infos, 0.3, 0.7)
    return mask


# ---------------------------------------------------------------------------------------------
# K1: drs_blend_step_known
# ---------------------------------------------------------------------------------------------
ANCESTRAL_T = (1499, 700, 2, 1)
DDIM_MOVES = ((49, 42), (1499, 1469), (7, 1), (1, 0), (1499, 0))


@pytest.mark.parametrize("kind", ["linear", "cosine"])
def test_blend_step_known_kernel(dev, kind):
    """drs_blend_step_known on the five geometries of test_gpu_tile_chain.py, masks of 1 and C bands holding both kinds, the
    moves of the two step-kernel tests.  Bit-equal: two calls; the unknown elements and `blend_step_` without `known`; the
    whole tensor under an all-zero mask; the known elements and `known` at t_prev == 0, and `inpaint_step_` on the same
    `known` / noise above it.  Float64 oracle (`inpaint_oracle.move` on the float64 blend): normalised error <= 1e-6 on each
    branch - unknown / max(|A x| + |B eps| + |sigma z|) as test_blend_step_kernel_vs_float64_oracle, known / max(|a known| +
    |b z|) as test_inpaint_step_kernel_vs_float64_oracle.  Measured on MI355X: unknown 1.3e-7 (both tables), known 8.0e-8
    (linear) / 8.4e-8 (cosine)."""
    from diffusionremotesensing_amd import hip_ops
    T = 1500
    alpha, ah, beta = D.schedule(kind, T)
    a_d, ah_d, b_d = alpha.to(dev), ah.to(dev), beta.to(dev)
    worst = [0.0, 0.0]
    for (h, w, ps, st, m, C) in GEOMETRIES:
        infos, _ = A.tile_infos(h, w, ps, st, m)
        S, Hs, Ws = ps * m, h * m, w * m
        wt = A.gaussian_weight(S, S)
        x, z, known = _randn(1, (1, C, Hs, Ws)), _randn(2, (1, C, Hs, Ws)), _randn(4, (1, C, Hs, Ws))
        eps_tiles = _randn(3, (len(infos), C, S, S))
        eps64 = TC.blend(eps_tiles, infos, wt, Hs, Ws)[None]
        org = hip_ops.tile_origins([(i[0], i[2]) for i in infos], S, Hs, Ws, dev)
        xd, zd, ed, wd, kd = x.to(dev), z.to(dev), eps_tiles.to(dev), wt.to(dev), known.to(dev)
        cases = [(t, None, 0.0) for t in ANCESTRAL_T] + [(t, tp, eta) for (t, tp) in DDIM_MOVES for eta in (0.0, 0.5, 1.0)]
        for Cm in sorted({1, C}):
            mask = (torch.rand((1, Cm, Hs, Ws), generator=torch.Generator().manual_seed(50 + Cm)) < 0.5).to(torch.uint8)
            assert 0 < int(mask.sum()) < mask.numel()
            md = mask.to(dev)
            mfull = mask.bool().expand_as(x)
            mdfull = md.bool().expand_as(xd)
            for t, tp, eta in cases:
                tag = (kind, (h, w, ps, st, m, C), Cm, t, tp, eta)
                to = t - 1 if tp is None else tp  # the level the move ends at
                noise, noise_d = (z, zd[0]) if to > 0 else (None, None)
                if tp is None:
                    form = {"alpha": a_d, "beta": b_d}
                    cA, cB, sigma = I.ancestral_coefficients(t, alpha, ah, beta)
                    want = I.move(x, eps64, noise, known, mask, t, to, ah, alpha=alpha, beta=beta)
                    plain_noise = noise_d
                else:
                    form = {"t_prev": tp, "eta": eta}
                    cA, cB, sigma = O.coefficients(t, tp, eta, ah)
                    want = I.move(x, eps64, noise, known, mask, t, tp, ah, eta=eta)
                    plain_noise = noise_d if eta > 0 else None  # the plain kernel takes no noise at eta = 0
                outs = [hip_ops.blend_step_(xd[0].clone(), ed, org, wd, noise_d, t, alpha_hat=ah_d, known=kd[0], known_mask=md[0],
                                            **form) for _ in range(2)]
                assert torch.equal(outs[0], outs[1]), tag
                plain = hip_ops.blend_step_(xd[0].clone(), ed, org, wd, plain_noise, t, alpha_hat=ah_d, **form)
                assert torch.equal(outs[0][~mdfull[0]], plain[~mdfull[0]]), tag
                zero = hip_ops.blend_step_(xd[0].clone(), ed, org, wd, noise_d, t, alpha_hat=ah_d, known=kd[0],
                                           known_mask=torch.zeros_like(md[0]), **form)
                assert torch.equal(zero, plain), tag
                if to == 0:
                    assert torch.equal(outs[0][mdfull[0]], kd[0][mdfull[0]]), tag
                else:
                    ref = hip_ops.inpaint_step_(xd.clone(), torch.zeros_like(xd), zd, kd, md, t, alpha_hat=ah_d, **form)
                    assert torch.equal(outs[0][mdfull[0]], ref[0][mdfull[0]]), tag
                got = outs[0].cpu().double()[None]
                scale_u = (cA * x.double()).abs() + (cB * eps64).abs()
                if noise is not None and sigma > 0:
                    scale_u = scale_u + (sigma * z.double()).abs()
                ka, kb = I.known_coefficients(to, ah) if to > 0 else (1.0, 0.0)
                scale_k = (ka * known.double()).abs() + (kb * z.double()).abs()
                err_u = ((got - want)[~mfull].abs().max() / scale_u.max()).item()
                err_k = ((got - want)[mfull].abs().max() / scale_k.max()).item()
                worst[0], worst[1] = max(worst[0], err_u), max(worst[1], err_k)
                assert err_u <= 1e-6 and err_k <= 1e-6, (tag, err_u, err_k, cA, cB, sigma, ka, kb)
    print(f"blend step known kernel [{kind}]: worst normalised error unknown {worst[0]:.3e} known {worst[1]:.3e}")


def test_blend_step_known_counts_uncovered_pixels(dev):
    """A scene whose right half no tile covers: counted by every call (the counter is not reset), whatever the mask says."""
    from diffusionremotesensing_amd import hip_ops
    _, ah, _ = D.schedule("cosine", 50)
    ah_d = ah.to(dev)
    S = 8
    scene = torch.zeros((1, 8, 16), device=dev)
    eps = torch.zeros((1, 1, S, S), device=dev)
    wt = A.gaussian_weight(S, S).to(dev)
    org = hip_ops.tile_origins([(0, 0)], S, 8, 16, dev)
    known = torch.full((1, 8, 16), 0.25, device=dev)
    mask = torch.zeros((1, 8, 16), dtype=torch.uint8, device=dev)
    mask[:, :, 4:12] = 1
    unc = torch.zeros(1, dtype=torch.int32, device=dev)
    hip_ops.blend_step_(scene, eps, org, wt, torch.zeros_like(scene), 10, alpha_hat=ah_d, t_prev=5, uncovered=unc, known=known,
                        known_mask=mask)
    hip_ops.blend_step_(scene, eps, org, wt, None, 5, alpha_hat=ah_d, t_prev=0, uncovered=unc, known=known, known_mask=mask)
    assert int(unc.item()) == 2 * 8 * 8
    assert torch.isfinite(scene[:, :, :8]).all() and torch.equal(scene[:, :, 4:12], known[:, :, 4:12])


# ---------------------------------------------------------------------------------------------
# K2: drs_aggregate_tiles_known
# ---------------------------------------------------------------------------------------------
def _blend_fp32(tiles, infos, weight, height, width):
    """`aggregation_oracle.aggregate` before its clamp: the sequential fp32 `+=` in tile order and the division."""
    C = tiles.shape[1]
    im = torch.zeros((C, height, width), dtype=torch.float32)
    cnt = torch.zeros((C, height, width), dtype=torch.float32)
    for i, (y0, y1, x0, x1) in enumerate(infos):
        im[:, y0:y1, x0:x1] += tiles[i] * weight
        cnt[:, y0:y1, x0:x1] += weight
    return im / cnt


def test_aggregate_tiles_known_kernel(dev):
    """drs_aggregate_tiles_known on the five geometries, tiles around [0, 1] as in test_aggregate_tiles_kernel.  Clamp (0, 1)
    without known pixels, and its unknown pixels with them: the bits of `aggregate_tiles`.  Clamp (-1, 1): the bits of the
    clamp of the un-clamped output.  Un-clamped: within 2.4e-7 of the oracle's sequential fp32 blend, the bar of
    test_aggregate_tiles_kernel (values in [-0.5, 1.5]: 2 ulp).  Known pixels: `known` under the clamp, exactly."""
    from diffusionremotesensing_amd import hip_ops, synthetic
    for (h, w, ps, st, m, C) in GEOMETRIES:
        infos, _ = A.tile_infos(h, w, ps, st, m)
        S, Hs, Ws = ps * m, h * m, w * m
        tiles = synthetic.tensor_uniform(f"aggknown.{h}.{w}", (len(infos), C, S, S), 0, -0.5, 1.5)
        wt = A.gaussian_weight(S, S)
        origins = [(i[0], i[2]) for i in infos]
        td, wd = tiles.to(dev), wt.to(dev)
        plain = hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws)
        raw = hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws, clamp=None)
        want = _blend_fp32(tiles, infos, wt, Hs, Ws)
        assert torch.equal(want.clamp(0, 1), A.aggregate(tiles, infos, wt, Hs, Ws)[0])  # the helper is the oracle's blend
        assert (raw.cpu() - want).abs().max().item() <= 2.4e-7, (h, w, (raw.cpu() - want).abs().max())
        assert raw.min().item() < 0 and raw.max().item() > 1
        assert torch.equal(hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws, clamp=(-1.0, 1.0)), raw.clamp(-1, 1)), (h, w)
        assert torch.equal(raw.clamp(0, 1), plain), (h, w)
        known = (3.0 * _randn(7, (C, Hs, Ws))).to(dev)  # beyond every clamp range used here
        for Cm in sorted({1, C}):
            mask = (torch.rand((Cm, Hs, Ws), generator=torch.Generator().manual_seed(60 + Cm)) < 0.5).to(torch.uint8).to(dev)
            mfull = mask.bool().expand(C, -1, -1)
            assert mfull.any() and not mfull.all()
            for clamp, lim in (((0.0, 1.0), lambda v: v.clamp(0, 1)), ((-1.0, 1.0), lambda v: v.clamp(-1, 1)), (None, lambda v: v)):
                got = hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws, clamp=clamp, known=known, known_mask=mask)
                assert torch.equal(got[mfull], lim(known)[mfull]), (h, w, Cm, clamp)
                assert torch.equal(got[~mfull], lim(raw)[~mfull]), (h, w, Cm, clamp)
                if clamp == (0.0, 1.0):
                    assert torch.equal(got[~mfull], plain[~mfull])
    with pytest.raises(AssertionError):  # a hole between tiles is counted whether its pixels are known or not
        hip_ops.aggregate_tiles(td[:1], [(0, 0)], wd, 2 * S, 2 * S, clamp=None, known=torch.zeros((C, 2 * S, 2 * S), device=dev),
                                known_mask=torch.ones((1, 2 * S, 2 * S), dtype=torch.uint8, device=dev))


# ---------------------------------------------------------------------------------------------
# K3: rejections
# ---------------------------------------------------------------------------------------------
def test_known_ops_reject_bad_arguments(dev):
    from diffusionremotesensing_amd import hip_ops
    alpha, ah, beta = D.schedule("cosine", 50)
    a_d, ah_d, b_d = alpha.to(dev), ah.to(dev), beta.to(dev)
    S, C, Hs, Ws = 8, 2, 8, 16
    scene = torch.zeros((C, Hs, Ws), device=dev)
    eps = torch.zeros((2, C, S, S), device=dev)
    wt = A.gaussian_weight(S, S).to(dev)
    org = hip_ops.tile_origins([(0, 0), (0, 8)], S, Hs, Ws, dev)
    z, kn = torch.zeros_like(scene), torch.zeros_like(scene)
    m1 = torch.zeros((1, Hs, Ws), dtype=torch.uint8, device=dev)
    ddim = {"alpha_hat": ah_d, "t_prev": 5, "eta": 0.0}

    def step(noise=z, known=kn, mask=m1, t=10, **kw):
        return hip_ops.blend_step_(scene, eps, org, wt, noise, t, known=known, known_mask=mask, **(kw or ddim))
    step()  # the good call
    # above level 0 the known pixels need z whatever eta is, in both forms
    with pytest.raises(RuntimeError, match="needs a noise tensor"):
        step(noise=None)
    with pytest.raises(RuntimeError, match="needs a noise tensor"):
        step(noise=None, t=2, alpha_hat=ah_d, alpha=a_d, beta=b_d)
    step(noise=None, alpha_hat=ah_d, t_prev=0, eta=1.0)
    step(noise=None, t=1, alpha_hat=ah_d, alpha=a_d, beta=b_d)
    with pytest.raises(RuntimeError, match="known without known_mask"):
        step(mask=None)
    with pytest.raises(RuntimeError, match="known_mask without known"):
        step(known=None)
    with pytest.raises(RuntimeError, match=r"known_mask \(3, 8, 16\)"):  # neither 1 nor C bands
        step(mask=torch.zeros((3, Hs, Ws), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="known_mask"):
        step(mask=torch.zeros((1, Hs, Ws + 4), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="known_mask must be torch.uint8"):
        step(mask=m1.float())
    with pytest.raises(RuntimeError, match=r"known \(2, 8, 12\)"):
        step(known=torch.zeros((C, Hs, Ws - 4), device=dev))
    with pytest.raises(RuntimeError, match="known is on cpu"):
        step(known=kn.cpu())
    with pytest.raises(RuntimeError, match="ROCm"):
        step(alpha_hat=ah, t_prev=5)  # the table must live on the device
    with pytest.raises(RuntimeError, match="known pixels"):
        step(noise=None, alpha_hat=ah_d, t_prev=5, hist=torch.zeros_like(scene))
    tiles = torch.zeros((2, C, S, S), device=dev)
    agg = {"known": kn, "known_mask": m1}
    hip_ops.aggregate_tiles(tiles, [(0, 0), (0, 8)], wt, Hs, Ws, clamp=None, **agg)
    with pytest.raises(RuntimeError, match="known without known_mask"):
        hip_ops.aggregate_tiles(tiles, [(0, 0), (0, 8)], wt, Hs, Ws, known=kn)
    with pytest.raises(RuntimeError, match=r"known_mask \(3, 8, 16\)"):
        hip_ops.aggregate_tiles(tiles, [(0, 0), (0, 8)], wt, Hs, Ws, known=kn,
                                known_mask=torch.zeros((3, Hs, Ws), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match=r"known \(2, 8, 12\)"):
        hip_ops.aggregate_tiles(tiles, [(0, 0), (0, 8)], wt, Hs, Ws, known=kn[:, :, :12].contiguous(), known_mask=m1)
    with pytest.raises(ValueError, match="clamp"):
        hip_ops.aggregate_tiles(tiles, [(0, 0), (0, 8)], wt, Hs, Ws, clamp=(1.0, 0.0))


# ---------------------------------------------------------------------------------------------
# C1: a one-tile scene is `sample_known`
# ---------------------------------------------------------------------------------------------
def _assert_ulps_per_move(got, want, moves, what):
    err = (got.double() - want.double()).abs().max().item()
    per_move = err / (ULP * want.abs().max().item()) / moves
    print(f"{what}: max abs difference {err:.3e} = {per_move:.2f} ulp of max |x| per move over {moves} moves")
    assert torch.isfinite(got).all()
    assert per_move <= ULPS_PER_STEP, (what, err, per_move)


@pytest.mark.parametrize("S,eta,resample,jump", [(None, 0.0, 1, 1), (5, 1.0, 2, 2)])
def test_one_tile_scene_agrees_with_sample_known(dev, seeded_sd, S, eta, resample, jump):
    """LR 32 x 32, x2, T = 8, exact fp32: the joint chain of a scene one tile covers against `Diffusion.sample_known` with the
    same draws, <= ULPS_PER_STEP (test_gpu_tile_chain.py: the blended eps of a pixel one tile covers is (w e) / w, 1 ulp from
    e, allowed a gain of 8 through the remaining forwards) per move, forward jumps counted as moves.  Measured on MI355X: 0.30
    ulp per move (ancestral, 7 moves), 0.38 (DDIM S = 5, eta 1, resample 2, jump 2: 11 moves)."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.sampling import chain_moves
    T = 8
    m = _sr_model(dev, seeded_sd, "mfma_f32")
    d = _sr_diffusion(m, dev, T)
    img = synthetic.tensor_uniform("tileknown.one", (1, 3, 32, 32)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 32, 2, d, dev)
    assert tiler.patches_sr_infos == [(0, 64, 0, 64)]
    known = synthetic.tensor_uniform("tileknown.one.known", (3, 64, 64))
    mask = _scene_mask(tiler.patches_sr_infos, 64, 64)
    kw = {"sampling_steps": S, "eta": eta, "resample": resample, "jump": jump}
    got = tiler.sample_scene(noise_source=replay_noise_source(78), known=known, known_mask=mask, **kw).cpu()
    assert m.training  # the samplers' side effect
    m.eval()
    want = d.sample_known(1, m, img[0], known, mask, input_channels=3, noise_source=replay_noise_source(78), **kw).cpu()[0]
    assert got.shape == (3, 64, 64)
    full = mask[None].expand(3, -1, -1)
    assert torch.equal(got[full], known[full]) and torch.equal(want[full], known[full])
    _assert_ulps_per_move(got, want, len(chain_moves(T, S, resample, jump)), f"one tile S={S} resample={resample}")


# ---------------------------------------------------------------------------------------------
# C2: the super-resolution joint chain against the float64 oracle
# ---------------------------------------------------------------------------------------------
# Max-abs error of the un-clamped scene against the float64 oracle chain, per chain (T, S, eta, resample, jump): (exact fp32,
# split bf16) - 10 x the error measured on MI355X (the same for both tile_batch settings), the convention for chains through
# untrained weights, the chain without resampling at most CHAIN_BOUNDS[(8, None, 0.0)] of test_gpu_tile_chain.py:
#   ancestral T = 8                                     1.905e-5 / 5.308e-4   on a state of max |x| =  40
#   DDIM T = 50, S = 10, eta 0.5, resample 2, jump 2    1.541e-3 / 3.624e-2   on a state of max |x| = 734  (18 forwards)
# Relative to max |x|: 4.8e-7 / 1.3e-5 and 2.1e-6 / 4.9e-5, the figures of the chains without known pixels there.
KNOWN_CHAINS = [(8, None, 0.0, 1, 1), (50, 10, 0.5, 2, 2)]
KNOWN_CHAIN_BOUNDS = {(8, None, 0.0, 1, 1): (min(1.9e-4, CHAIN_BOUNDS[(8, None, 0.0)][0]), min(5.3e-3, CHAIN_BOUNDS[(8, None, 0.0)][1])),
                      (50, 10, 0.5, 2, 2): (1.5e-2, 3.6e-1)}


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
@pytest.mark.parametrize("T,S,eta,resample,jump", KNOWN_CHAINS)
def test_joint_chain_with_known_pixels_vs_float64_oracle(dev, seeded_sd, impl, T, S, eta, resample, jump):
    """The scene of test_joint_chain_vs_float64_oracle (LR 48x56, patch 32, stride 16, x2: six overlapping tiles) with a block
    mask, through `sample_scene(known=, known_mask=)` with tile_batch 16 and 4, against the float64 oracle chain over the fp32
    oracle UNet.  The known pixels come back exactly and the others differ from `known`; the two chunkings agree to the bit on
    the exact-fp32 kernels."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    m = _sr_model(dev, seeded_sd, impl)
    d = _sr_diffusion(m, dev, T)
    img = synthetic.tensor_uniform("g10.img", (1, 3, 48, 56))
    tiler = split_aggregation_sampling(img.to(dev), 32, 16, 2, d, dev)
    infos, lr_origins = A.tile_infos(48, 56, 32, 16, 2)
    assert [tuple(i) for i in tiler.patches_sr_infos] == infos and len(infos) == 6
    known = synthetic.tensor_uniform("tileknown.sr.known", (3, 96, 112))
    mask = _scene_mask(infos, 96, 112)
    full = mask[None].expand(3, -1, -1)
    seed = 5000 + T + (S or 0) + resample
    key = (T, S, eta, resample, jump)

    def oracle():
        lr_tiles = torch.stack([img[0, :, y0:y0 + 32, x0:x0 + 32] for (y0, x0) in lr_origins])
        return TK.chain(TC.unet_eps_fn(U.OracleUNet(seeded_sd), lr_tiles, 2), 3, 96, 112, infos, A.gaussian_weight(64, 64), T,
                        D.schedule("cosine", T), replay_noise_source(seed), known, mask, S, eta, resample, jump)
    if key not in _ORACLE:
        _ORACLE[key] = oracle()
    want = _ORACLE[key]
    assert torch.equal(want[full], known.double()[full])
    outs = {}
    for tile_batch in (16, 4):
        tiler.tile_batch = tile_batch
        got = tiler.sample_scene(noise_source=replay_noise_source(seed), sampling_steps=S, eta=eta, known=known, known_mask=mask,
                                 resample=resample, jump=jump).cpu()
        m.eval()
        assert got.shape == (3, 96, 112) and torch.isfinite(got).all()
        assert torch.equal(got[full], known[full])
        assert (got - known)[~full].abs().min().item() > 0
        err = (got.double() - want).abs().max().item()
        top = want.abs().max().item()
        print(f"joint chain with known pixels T={T} S={S} eta={eta} resample={resample} jump={jump} [{impl}] "
              f"tile_batch={tile_batch}: max abs error {err:.3e} = {err / top:.2e} of max |x| {top:.2f}")
        assert err <= KNOWN_CHAIN_BOUNDS[key][impl == "mfma_bf16x3"], (impl, key, tile_batch, err)
        outs[tile_batch] = got
    if impl == "mfma_f32":
        assert torch.equal(outs[16], outs[4])


# ---------------------------------------------------------------------------------------------
# C3: a SAR -> NDVI scene
# ---------------------------------------------------------------------------------------------
# SAR 2 x 96 x 112 -> NDVI 1 x 96 x 112, patch 64, stride 32, magnification 1: six tiles, the clamped last column at x0 = 48
SAR = {"T": 30, "S": 10, "eta": 0.5, "resample": 2, "jump": 2}
# (exact fp32, split bf16): 10 x the error measured on MI355X against the float64 oracle chain, 7.322e-3 / 1.686e-1 on a state
# of max |x| = 997 (7.3e-6 / 1.7e-4 of it; 18 forwards of untrained weights)
SAR_CHAIN_BOUNDS = (7.3e-2, 1.7)


def _sar_scene(dev, sd, impl):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.train_diffusion_SAR_TO_NDVI import Diffusion
    m = _sar_model(dev, sd, impl)
    d = Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=SAR["T"], device=dev, image_size=64)
    sar = synthetic.tensor_uniform("tileknown.sar", (1, 2, 96, 112))
    tiler = split_aggregation_sampling(sar.to(dev), 64, 32, 1, d, dev, out_channels=1, clamp=None)
    infos, origins = A.tile_infos(96, 112, 64, 32, 1)
    assert [tuple(i) for i in tiler.patches_sr_infos] == infos and len(infos) == 6 and (0, 48) in origins
    known = synthetic.tensor_uniform("tileknown.sar.known", (1, 96, 112), 0, -1.0, 1.0)
    mask = _scene_mask(infos, 96, 112)
    return m, tiler, sar, infos, origins, known, mask


@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
def test_sar_scene_per_step_vs_float64_oracle(dev, seeded_sd_sar, impl):
    """`sample_scene` of the SAR -> NDVI model (T = 30, S = 10, eta 0.5, resample 2, jump 2) against the float64 oracle chain
    over OracleUNetSAR; `aggregation_sampling(aggregation="per_step")` with clamp=None returns that state, values outside
    [0, 1] included, with the known pixels exactly `known`."""
    m, tiler, sar, infos, origins, known, mask = _sar_scene(dev, seeded_sd_sar, impl)
    kw = {"sampling_steps": SAR["S"], "eta": SAR["eta"], "resample": SAR["resample"], "jump": SAR["jump"]}

    def oracle():
        model = U.OracleUNetSAR(seeded_sd_sar)
        sar_tiles = torch.stack([sar[0, :, y0:y0 + 64, x0:x0 + 64] for (y0, x0) in origins])

        def eps_fn(x_tiles, t, rng):
            k0, k1 = rng
            return model(x_tiles, torch.full((k1 - k0,), t, dtype=torch.long), sar_tiles[k0:k1])
        return TK.chain(eps_fn, 1, 96, 112, infos, A.gaussian_weight(64, 64), SAR["T"], D.schedule("cosine", SAR["T"]),
                        replay_noise_source(616), known, mask, SAR["S"], SAR["eta"], SAR["resample"], SAR["jump"])
    if "sar" not in _ORACLE:
        _ORACLE["sar"] = oracle()
    want = _ORACLE["sar"]
    got = tiler.sample_scene(noise_source=replay_noise_source(616), known=known, known_mask=mask, **kw).cpu()
    m.eval()
    assert got.shape == (1, 96, 112) and torch.isfinite(got).all()
    err = (got.double() - want).abs().max().item()
    top = want.abs().max().item()
    print(f"SAR scene per_step [{impl}]: max abs error {err:.3e} = {err / top:.2e} of max |x| {top:.2f}")
    assert err <= SAR_CHAIN_BOUNDS[impl == "mfma_bf16x3"], (impl, err)
    out = tiler.aggregation_sampling(noise_source=replay_noise_source(616), aggregation="per_step", known=known, known_mask=mask,
                                     **kw).cpu()
    assert out.shape == (1, 1, 96, 112) and torch.equal(out[0], got)
    assert torch.equal(out[0][mask[None]], known[mask[None]])
    assert ((out < 0) | (out > 1)).any()  # nothing clamps an NDVI scene to [0, 1]


def test_sar_scene_final_mode_is_the_blend_of_sample_known_tiles(dev, seeded_sd_sar):
    """aggregation="final" with known pixels: the float64 blend of the GPU's own `sample_known` tiles (`sample_tiles`, here in
    chunks of four), the known pixels replaced by `known`, at the bar of the aggregate kernel (2.4e-7 on values in [0, 1],
    scaled to the largest blended value), un-clamped.  Measured on MI355X: 1.66e-4 on max |x| = 1100 (1.5e-7 of it)."""
    m, tiler, sar, infos, origins, known, mask = _sar_scene(dev, seeded_sd_sar, "mfma_f32")
    tiler.tile_batch = 4
    kw = {"sampling_steps": SAR["S"], "eta": SAR["eta"], "resample": SAR["resample"], "jump": SAR["jump"]}

    def src(tile, i, shape):  # one fixed draw per (tile, level): the resampling asks a level more than once
        return _randn(7000 + 100 * tile + i, shape)
    tiles = tiler.sample_tiles(noise_source=src, known=known, known_mask=mask, **kw).cpu()
    m.eval()
    assert tiles.shape == (6, 1, 64, 64) and torch.isfinite(tiles).all()
    for k, (y0, y1, x0, x1) in enumerate(infos):  # every tile chain kept its crop of the known pixels
        win = mask[None, y0:y1, x0:x1]
        assert torch.equal(tiles[k][win], known[:, y0:y1, x0:x1][win])
    out = tiler.aggregation_sampling(noise_source=src, known=known, known_mask=mask, **kw).cpu()
    assert out.shape == (1, 1, 96, 112)
    want = TC.blend(tiles, infos, A.gaussian_weight(64, 64), 96, 112)
    want = torch.where(mask[None], known.double(), want)
    top = max(1.0, want.abs().max().item())
    err = (out[0].double() - want).abs().max().item()
    print(f"SAR scene final mode: max abs error {err:.3e} against the float64 blend, max |x| {top:.2f}")
    assert err <= 2.4e-7 * top, (err, top)
    assert torch.equal(out[0][mask[None]], known[mask[None]])
    assert ((out < 0) | (out > 1)).any()


# ---------------------------------------------------------------------------------------------
# C4: nothing known is the plain joint chain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,eta", [(None, 0.0), (5, 0.0)])
def test_all_zero_mask_is_the_plain_joint_chain_bit_for_bit(dev, seeded_sd, S, eta):
    """Same replay seed, nothing known, no resampling: the bits of `sample_scene` without `known` (an eta = 0 chain with known
    pixels draws at every move, the plain one only x_T; the unknown elements read none of those draws)."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T = 8
    m = _sr_model(dev, seeded_sd, "mfma_f32")
    d = _sr_diffusion(m, dev, T)
    img = synthetic.tensor_uniform("g10.img", (1, 3, 48, 56)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)
    plain = tiler.sample_scene(noise_source=replay_noise_source(91), sampling_steps=S, eta=eta).cpu()
    m.eval()
    zero = tiler.sample_scene(noise_source=replay_noise_source(91), sampling_steps=S, eta=eta, known=torch.zeros((3, 96, 112)),
                              known_mask=torch.zeros((96, 112), dtype=torch.bool)).cpu()
    assert torch.isfinite(plain).all() and torch.equal(plain, zero)


# ---------------------------------------------------------------------------------------------
# C5: determinism, the batch dimension, the command line
# ---------------------------------------------------------------------------------------------
def test_known_scene_is_deterministic_and_broadcasts_over_the_batch(dev, seeded_sd):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    T = 8
    m = _sr_model(dev, seeded_sd, "mfma_f32")
    d = _sr_diffusion(m, dev, T)
    img = synthetic.tensor_uniform("tileknown.batch", (2, 3, 32, 48)).to(dev)
    tiler = split_aggregation_sampling(img, 32, 16, 2, d, dev)
    known = synthetic.tensor_uniform("tileknown.batch.known", (3, 64, 96), 0, -0.5, 1.5)
    mask = TK.block_mask(MASK_SEED, 64, 96)
    full = mask[None].expand(3, -1, -1)
    kw = {"sampling_steps": 4, "eta": 1.0, "resample": 2, "jump": 2, "known": known, "known_mask": mask}
    outs = []
    for _ in range(2):
        outs.append(tiler.aggregation_sampling(noise_source=replay_noise_source(5), aggregation="per_step", **kw).cpu())
        m.eval()
    assert outs[0].shape == (2, 3, 64, 96)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0][0], outs[0][1])
    assert torch.equal(outs[0][0][full], known.clamp(0, 1)[full])  # the known pixels, clamped like the rest
    assert outs[0].min().item() >= 0 and outs[0].max().item() <= 1
    scene = tiler.sample_scene(noise_source=replay_noise_source(5), **kw).cpu()
    m.eval()
    assert torch.equal(outs[0][0], scene.clamp(0, 1)) and torch.equal(scene[full], known[full])

    def src(tile, i, shape):
        return _randn(8000 + 100 * tile + i, shape)
    final = tiler.aggregation_sampling(noise_source=src, **kw).cpu()
    assert final.shape == (2, 3, 64, 96) and torch.equal(final[0], final[1])
    assert torch.equal(final[0][full], known.clamp(0, 1)[full])


def test_cli_sar_to_ndvi_round_trip(dev, tmp_path):
    """`Aggregation_Sampling --task sar_to_ndvi --known_path ... --aggregation per_step` on temporary files (T = 8, untrained
    weights): the written scene is (NDVI_channels, H, W), un-clamped by default, and its known pixels are the input's."""
    from diffusionremotesensing_amd import Aggregation_Sampling as AS
    from diffusionremotesensing_amd import synthetic
    sar = synthetic.tensor_uniform("tileknown.cli.sar", (2, 64, 96))
    known = synthetic.tensor_uniform("tileknown.cli.known", (1, 64, 96), 0, -1.0, 1.0)
    mask = TK.block_mask(MASK_SEED, 64, 96)
    torch.save(sar, tmp_path / "sar.pt")
    torch.save(known, tmp_path / "known.pt")
    torch.save(mask, tmp_path / "mask.pt")
    argv = ["--task", "sar_to_ndvi", "--model_name", "m", "--UNet_type", "Residual Attention UNet", "--device", str(dev),
            "--noise_steps", "8", "--model_input_size", "64", "--magnification_factor", "1", "--patch_size", "64", "--stride", "32",
            "--img_lr_path", str(tmp_path / "sar.pt"), "--destination_path", str(tmp_path / "out.pt"), "--known_path",
            str(tmp_path / "known.pt"), "--known_mask_path", str(tmp_path / "mask.pt"), "--aggregation", "per_step"]
    a = AS.build_arg_parser().parse_args(argv)
    a.snapshot_folder_path = str(tmp_path)
    AS.launch(a)
    out = torch.load(tmp_path / "out.pt")
    assert out.shape == (1, 64, 96) and torch.isfinite(out).all()
    assert torch.equal(out[mask[None]], known[mask[None]])
    assert (out[~mask[None]] != known[~mask[None]]).any()
