"""The sensor-MTF degradation on the device: `hip_ops.fir_decimate` and the per-band forms of the three
projection entries against the float64 oracle (tests/mtf_oracle.py, tests/consistency_oracle.py) within its bounds,
repeatability, the one-operator stack against the 2-D call, projected chains under three band operators, `DeviceMTFFeed`,
`Diffusion.sample` / `evaluate` with Degradation_type "MTF", and the tiler's scene projection."""
import numpy as np
import pytest
import torch

import consistency_oracle as CO
import mtf_oracle as MO
from guard import bits_equal
from oracle import diffusion_oracle as D

pytestmark = pytest.mark.gpu

# (B, C, H, W, m), gains: non-square; 16 bands with 16 gains; trailing rows and W % 4 != 0 (the element-wise loads); L = 19 > H
# (every tap clamps); m = 8 at its smallest tile; several tiles per axis with a ragged last one
FIR_CASES = [((2, 3, 24, 24, 2), (0.35, 0.3, 0.35)), ((1, 1, 20, 28, 4), (0.2,)),
             ((1, 16, 32, 32, 2), tuple(np.linspace(0.05, 0.6, 16).round(4).tolist())), ((1, 2, 70, 66, 3), (0.6, 0.1)),
             ((1, 1, 8, 16, 8), (0.05,)), ((1, 1, 64, 64, 8), (0.3,)), ((1, 3, 136, 136, 2), (0.4, 0.4, 0.05))]
T = 50
LEVELS = [1, 7, T // 2, T - 1]
_FIR, _PROJ = {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _within(got, want_bound, what):
    want, bound = want_bound
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| {err.max():.3e}, max bound {bound.max():.3e}, worst err / bound {ratio:.3e}")
    assert np.isfinite(err).all() and ratio <= 1.0, what


def _image(shape, g, spread=0.05):
    B, Cn, H, W = shape
    yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    return (0.5 + 0.3 * torch.sin(6.0 * xx + 1.0) * torch.cos(5.0 * yy))[None, None] + spread * torch.randn(shape, generator=g)


def _fir_case(shape, gains):
    """Inputs and the oracle's results of one FIR case, computed once and shared (also by the guard and stream-order files)."""
    key = (shape, gains)
    if key in _FIR:
        return _FIR[key]
    B, Cn, H, W, m = shape
    rows, L, band_op = MO.band_taps(gains, m)
    g = torch.Generator().manual_seed(17 + H + 3 * W + Cn)
    x = _image((B, Cn, H, W), g).float()
    z = torch.randn((B, Cn, H // m, W // m), generator=g)
    sigma = torch.linspace(0.0, 0.3, Cn)  # large enough that the clamp acts
    plain = MO.fir_bands(x.double().numpy(), rows, rows, band_op, L, L, m)
    case = {"x": x, "z": z, "sigma": sigma, "rows": torch.from_numpy(rows).float(), "L": L, "band_op": band_op, "m": m,
            "plain": plain, "noisy": MO.epilogue(*plain, z.double().numpy(), sigma.double().numpy(), clamp=True),
            "clamped": MO.epilogue(*plain, clamp=True)}
    assert np.array_equal(case["rows"].double().numpy(), rows)  # the oracle's taps are fp32 numbers
    _FIR[key] = case
    return case


@pytest.mark.parametrize("shape,gains", FIR_CASES, ids=[str(c[0]) for c in FIR_CASES])
def test_fir_decimate_vs_float64_oracle(dev, shape, gains):
    from diffusionremotesensing_amd import consistency, hip_ops
    from diffusionremotesensing_amd.consistency import BandOperator
    c = _fir_case(shape, gains)
    B, Cn, H, W, m = shape
    x, rows, z, sigma = (c[k].to(dev) for k in ("x", "rows", "z", "sigma"))

    def run(**kw):
        return hip_ops.fir_decimate(x, rows, rows, c["L"], m, band_op=c["band_op"], **kw)
    got = run()
    assert tuple(got.shape) == (B, Cn, H // m, W // m)
    _within(got, c["plain"], f"fir_decimate {shape}")
    assert bits_equal(got, run())  # two calls, the same bits
    noisy = run(noise=z, sigma=sigma, clamp=True)
    _within(noisy, c["noisy"], f"fir_decimate + noise + clamp {shape}")
    assert float(noisy.min()) >= 0.0 and float(noisy.max()) <= 1.0 and bits_equal(noisy, run(noise=z, sigma=sigma, clamp=True))
    assert bits_equal(run(clamp=True), got.clamp(0.0, 1.0))
    # the dense operator of the projection is the same map: within its own (section 28) bound of the same oracle
    op = BandOperator.mtf((H, W), m, gains)
    assert op.band_op == c["band_op"]
    dense = consistency.degrade(x, op)
    proj = MO.BandProjection(H, W, m, gains, 0.01)
    want, bound = proj.degrade(c["x"].double().numpy())
    assert np.abs(want - c["plain"][0]).max() <= 1e-13  # (the two oracles agree: FIR and dense form of one operator)
    _within(dense, (c["plain"][0], bound), f"dense sep_apply {shape}")
    if Cn > 1:  # the default table: band b -> min(b, n_ops - 1)
        n_ops = rows.shape[0]
        default = hip_ops.fir_decimate(x, rows, rows, c["L"], m)
        want = MO.fir_bands(c["x"].double().numpy(), c["rows"].double().numpy(), c["rows"].double().numpy(),
                            [min(b, n_ops - 1) for b in range(Cn)], c["L"], c["L"], m)
        _within(default, want, f"fir_decimate, default table {shape}")


def test_fir_pointer_phase_and_separate_axes(dev):
    """A view that starts 4 bytes into its buffer takes the 4-byte loads: the same bits.  Different taps and lefts per axis."""
    from diffusionremotesensing_amd import hip_ops
    c = _fir_case(*FIR_CASES[0])
    x, rows = c["x"].to(dev), c["rows"].to(dev)
    want = hip_ops.fir_decimate(x, rows, rows, c["L"], 2, band_op=c["band_op"])
    buf = torch.zeros(x.numel() + 1, device=dev)
    buf[1:] = x.reshape(-1)
    shifted = buf[1:].view(x.shape)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert bits_equal(hip_ops.fir_decimate(shifted, rows, rows, c["L"], 2, band_op=c["band_op"]), want)
    ky, Ly = MO.taps(0.2, 2)
    kx, Lx = MO.taps(0.5, 2)
    got = hip_ops.fir_decimate(x, torch.from_numpy(ky).float().to(dev), torch.from_numpy(kx).float().to(dev), (Ly, Lx), 2)
    xn = c["x"].double().numpy()
    _within(got, (MO.fir(xn, ky, kx, Ly, Lx, 2), MO.fir_gamma(len(ky), len(kx)) * MO.fir_abs(xn, ky, kx, Ly, Lx, 2)), "separate axes")


# ---------------------------------------------------------------------------------------------
# per-band projection
# ---------------------------------------------------------------------------------------------
PROJ_CASES = [((2, 3, 24, 24, 2), (0.35, 0.3, 0.2), 0.01), ((2, 3, 24, 24, 2), (0.3, 0.3, 0.3), 0.0),
              ((2, 3, 24, 24, 2), (0.3, 0.3, 0.3), 0.01), ((1, 2, 20, 28, 4), (0.05, 0.05), 0.01)]


def _schedule():
    return D.schedule("cosine", T)


def _proj_case(shape, gains, damping):
    key = (shape, gains, damping)
    if key in _PROJ:
        return _PROJ[key]
    from diffusionremotesensing_amd.consistency import BandOperator
    B, Cn, H, W, m = shape
    op = BandOperator.mtf((H, W), m, gains)
    proj = MO.BandProjection(H, W, m, gains, damping)
    g = torch.Generator().manual_seed(29 + H + 3 * W + Cn)
    truth = _image((B, Cn, H, W), g)
    x0 = (truth + 0.1 * torch.randn((B, Cn, H, W), generator=g)).float()
    y = torch.from_numpy(proj.degrade(truth.double().numpy())[0]).float() + 0.01 * torch.randn((B, Cn) + op.lr_shape, generator=g)
    eps = torch.randn((B, Cn, H, W), generator=g)
    t = torch.tensor([LEVELS[(i + H) % len(LEVELS)] for i in range(B)])
    ah = _schedule()[1]
    a, s = ah[t].double().sqrt()[:, None, None, None], (1.0 - ah[t].double()).sqrt()[:, None, None, None]
    x = (a * x0.double() + s * eps.double()).float()
    n = {k: v.double().numpy() for k, v in (("x0", x0), ("y", y), ("eps", eps), ("x", x))}
    case = {"op": op, "proj": proj, "x0": x0, "y": y, "eps": eps, "x": x, "t": t, "ah": ah, "degrade": proj.degrade(n["x0"]),
            "project": proj.project(n["x0"], n["y"]), "project_eps": proj.project_eps(n["eps"], n["x"], ah[t].double().numpy(), n["y"])}
    _PROJ[key] = case
    return case


@pytest.mark.parametrize("shape,gains,damping", PROJ_CASES, ids=[f"{c[0]}-{c[1]}-d{c[2]}" for c in PROJ_CASES])
def test_band_entries_vs_float64_oracle(dev, shape, gains, damping):
    from diffusionremotesensing_amd import consistency, hip_ops
    c = _proj_case(shape, gains, damping)
    what = f"{shape} gains {gains} damping {damping}"
    projector = c["op"].projector(damping, dev)
    assert projector.D_y.dim() == 3 and projector.band_op == c["op"].band_op
    x0, y, eps, x, t, ah = (c[k].to(dev) for k in ("x0", "y", "eps", "x", "t", "ah"))
    lr = consistency.degrade(x0, c["op"])
    _within(lr, c["degrade"], f"degrade {what}")
    assert bits_equal(lr, consistency.degrade(x0, c["op"]))
    rm = consistency.lr_rmse(x0, y, c["op"]).double().cpu().numpy()
    assert np.allclose(rm, np.sqrt(((c["degrade"][0] - c["y"].double().numpy()) ** 2).mean(axis=(1, 2, 3))), rtol=1e-4, atol=1e-7)
    p = consistency.project(x0, y, projector)
    _within(p, c["project"], f"project {what}")
    assert bits_equal(p, consistency.project(x0, y, projector))
    assert bits_equal(consistency.project(x0, y, projector, strength=0.0), x0)  # strength 0: the identity, bit for bit
    in_place = x0.clone()
    assert consistency.project(in_place, y, projector, out=in_place) is in_place and bits_equal(in_place, p)
    yt = projector.prepare(y)
    e1 = hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector)
    _within(e1, c["project_eps"], f"project_eps {what}")
    assert bits_equal(e1, hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector))
    assert bits_equal(hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector, 0.0), eps)
    if damping == 0.0:  # the undamped projection lands on the observation, band by band
        got = p.double().cpu().numpy()
        for b, pr in enumerate(c["proj"].per_band):
            resid = np.abs(pr.degrade(got[:, b]) - c["y"].double().numpy()[:, b])
            assert (resid <= pr.degrade_abs(c["project"][1][:, b])).all(), (b, resid.max())


def test_one_operator_stack_is_the_2d_call(dev):
    """A 3-D stack with n_ops = 1 through the *_bands entries gives the bits of the plain entries, for all three."""
    import types
    from diffusionremotesensing_amd import hip_ops
    from diffusionremotesensing_amd.consistency import SeparableOperator
    c = _proj_case(*PROJ_CASES[2])
    one = SeparableOperator.mtf((24, 24), 2, 0.3)
    p2 = one.projector(0.01, dev)
    names = ("D_y", "D_x", "U_y", "U_x", "G", "Pt_y", "Pt_x")
    p3 = types.SimpleNamespace(**{k: getattr(p2, k)[None].contiguous() for k in names}, band_op=None)
    x0, y, eps, x, t, ah = (c[k].to(dev) for k in ("x0", "y", "eps", "x", "t", "ah"))
    A_y, A_x = one.matrices(dev)
    assert bits_equal(hip_ops.sep_apply(x0, A_y[None].contiguous(), A_x[None].contiguous()), hip_ops.sep_apply(x0, A_y, A_x))
    yt = hip_ops.sep_apply(y, p2.Pt_y, p2.Pt_x)
    assert bits_equal(hip_ops.sep_apply(y, p3.Pt_y, p3.Pt_x, band_op=[0, 0, 0]), yt)
    assert bits_equal(hip_ops.sep_project(x0, yt, p3, 0.8), hip_ops.sep_project(x0, yt, p2, 0.8))
    assert bits_equal(hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, p3, 0.8),
                      hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, p2, 0.8))
    # ... and the band operator of three equal gains (one shared operator) is that call too
    shared = c["op"].projector(0.01, dev)
    assert shared.D_y.shape[0] == 1 and bits_equal(hip_ops.sep_project(x0, shared.prepare(y), shared, 0.8), hip_ops.sep_project(x0, yt, p2, 0.8))


# ---------------------------------------------------------------------------------------------
# projected chains
# ---------------------------------------------------------------------------------------------
CHAIN_GAINS = (0.35, 0.2, 0.05)


class _Schedule:
    Degradation_type, magnification_factor, mtf_nyquist = "MTF", 2, CHAIN_GAINS

    def __init__(self, n_steps, dev, request):
        self.noise_steps, self.device, self.lr_consistency = n_steps, dev, request
        self.tables = D.schedule("cosine", n_steps)
        self.alpha, self.alpha_hat, self.beta = (v.to(dev) for v in self.tables)


class _Engine:
    def check_faults(self):
        pass


CHAINS = {"ddim4": (50, 4), "ancestral6": (7, None)}


@pytest.mark.parametrize("kind", list(CHAINS))
def test_projected_chain_under_three_band_operators(dev, kind):
    """Scripted predictions, damping 0: every band's fp32 chain stays within the oracle chain's running bound for that band's own
    operator (per plane, Frobenius norm), and the un-clamped result maps to the observation within the bound of its last move."""
    from diffusionremotesensing_amd import sampling
    from diffusionremotesensing_amd.consistency import LRConsistency
    n_steps, S = CHAINS[kind]
    shape = (2, 3, 24, 24)
    sch = _Schedule(n_steps, dev, LRConsistency(damping=0.0))
    levels = sampling.chain_levels(n_steps, S)
    assert len(levels) == (4 if S else 6)
    g = torch.Generator().manual_seed(13)
    scripted = {t: torch.randn(shape, generator=g) for t in levels}
    noise = {t: torch.randn(shape, generator=g) for t in levels + [n_steps]}
    y = 0.2 + 0.6 * torch.rand((2, 3, 12, 12), generator=g)
    order = iter(levels)
    got = sampling.sample_chain(sch, _Engine(), shape, lambda e, x, t, first: scripted[next(order)].to(dev), table_rows=2,
                                noise_source=lambda i, shp: noise[i], sampling_steps=S, lr_img=y)
    got = got.double().cpu().numpy()
    alpha, ah, beta = (v.double().numpy() for v in sch.tables)
    bands = MO.BandProjection(24, 24, 2, CHAIN_GAINS, 0.0)
    for b, proj in enumerate(bands.per_band):
        want, E, resid_bound = CO.chain(proj, y[:, b].double().numpy(), ah, levels, lambda t: scripted[t][:, b].double().numpy(),
                                        lambda t: noise[t][:, b].double().numpy(), noise[n_steps][:, b].double().numpy(),
                                        ancestral=S is None, alpha=alpha, beta=beta)
        err = np.sqrt(((got[:, b] - want) ** 2).sum(axis=(-2, -1), keepdims=True))
        print(f"{kind} band {b} (g = {CHAIN_GAINS[b]}): max |err| {np.abs(got[:, b] - want).max():.3e}, worst norm / bound {(err / E).max():.3e}")
        assert (err <= E).all()
        resid = np.abs(proj.degrade(got[:, b]) - y[:, b].double().numpy())
        print(f"{kind} band {b}: max |A_c x - y| {resid.max():.3e}, worst / bound {(resid / resid_bound).max():.3e}")
        assert (resid <= resid_bound).all()


# ---------------------------------------------------------------------------------------------
# the feed
# ---------------------------------------------------------------------------------------------
def _caches():
    rng = np.random.default_rng(5)
    u8 = torch.from_numpy(rng.integers(0, 256, (6, 3, 20, 20)).astype(np.uint8))
    dn = rng.integers(0, 12000, (6, 3, 20, 20)).astype(np.uint16)
    dn[:, :, 3:6, 4:9] = 777  # no-data pixels: all bands hold the marker
    dn[:, 1, 10, 10] = 777    # one band alone: data
    return u8, torch.from_numpy(dn)


@pytest.mark.parametrize("depth", [8, 16])
def test_feed_is_crop_then_fir(dev, depth):
    from diffusionremotesensing_amd import augment, hip_ops, mtf, radiometry
    u8, u16 = _caches()
    gains = (0.35, 0.2, 0.35)
    kw = dict(crop_size=16, augment="d4", augment_seed=3) if depth == 8 else {}
    table = [(0, 10000), (100, 12000), (0, 8000)]
    if depth == 8:
        feed = mtf.DeviceMTFFeed(u8.to(dev), 2, gains, batch_size=4, **kw)
    else:
        feed = mtf.DeviceMTFFeed(u16.to(dev), 2, gains, batch_size=4, data_range=table, nodata=777)
    assert len(feed) == 2 and feed.operator.band_op == [0, 1, 0]
    rows = torch.from_numpy(feed.taps).float().to(dev)
    seen = 0
    for lr, hr in feed:
        items = augment.upload_items(feed.last_items, dev)
        if depth == 8:
            want_hr = augment.crop_d4_u8_f32(u8.to(dev), torch.zeros(6, dtype=torch.int64, device=dev), items, 16)[0]
            stored = want_hr
        else:
            stored, want_hr = radiometry.crop_d4_u16_f32(u16.to(dev), items, 20, radiometry.device_table(radiometry.check_table(table, 3), dev), 777)
            assert torch.isnan(want_hr[:, :, 3:6, 4:9]).all() and not torch.isnan(want_hr[:, 1, 10, 10]).any()
            assert not torch.isnan(stored).any()
        want_lr = hip_ops.fir_decimate(stored, rows, rows, feed.left, 2, band_op=[0, 1, 0], clamp=True)
        assert bits_equal(hr, want_hr) and bits_equal(lr, want_lr)  # the LR image comes from the stored pixels
        assert tuple(lr.shape[1:]) == (3, hr.shape[-1] // 2, hr.shape[-1] // 2) and not torch.isnan(lr).any()
        seen += lr.shape[0]
    assert seen == 6
    x, y = feed.item(2)
    assert tuple(x.shape) == (3, y.shape[-1] // 2, y.shape[-1] // 2)


def test_feed_noise(dev):
    from diffusionremotesensing_amd import mtf
    u8, _ = _caches()

    def epoch(feed):
        return torch.cat([lr for lr, _ in feed])
    fixed = mtf.DeviceMTFFeed(u8.to(dev), 2, 0.3, noise="0.02,0.05,0.1", batch_size=4, shuffle=False, fixed=True, seed=9)
    quiet = mtf.DeviceMTFFeed(u8.to(dev), 2, 0.3, batch_size=4, shuffle=False, fixed=True)
    first = epoch(fixed)
    assert bits_equal(epoch(fixed), first)  # a fixed feed repeats its noise
    clean = epoch(quiet)
    d = (first - clean).double()
    inside = (clean > 0.3) & (clean < 0.7)  # away from the clamp the difference is the noise: its per-band deviation
    for b, s in enumerate((0.02, 0.05, 0.1)):
        got = float(d[:, b][inside[:, b]].std())
        print(f"band {b}: noise deviation {got:.4f} for sigma {s}")
        assert 0.8 * s < got < 1.2 * s
    drawn = mtf.DeviceMTFFeed(u8.to(dev), 2, 0.3, noise="0.02,0.05,0.1", batch_size=4, shuffle=False, seed=9)
    a, b = epoch(drawn), epoch(drawn)
    assert bits_equal(a, first) and not bits_equal(b, a)  # the same seed starts alike; an unfixed feed draws on
    other = mtf.DeviceMTFFeed(u8.to(dev), 2, 0.3, noise="0.02,0.05,0.1", batch_size=4, shuffle=False, seed=9, augment_rank=1)
    assert not bits_equal(epoch(other), first)  # each rank its own normals
    assert bits_equal(fixed.item(1)[0], clean[1]) and bits_equal(drawn.item(1)[0], clean[1])  # item: no noise


# ---------------------------------------------------------------------------------------------
# Diffusion.sample, evaluate and the tiler
# ---------------------------------------------------------------------------------------------
SAMPLE_GAINS = (0.35, 0.3, 0.2)


@pytest.fixture(scope="module")
def diffusion(dev, seeded_sd):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    return Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, magnification_factor=2, image_size=32,
                     Degradation_type="MTF", mtf_nyquist=SAMPLE_GAINS)


def _src(seed):
    return lambda i, shape: torch.randn(shape, generator=torch.Generator().manual_seed(seed + i))


def test_sample_with_the_attribute_off_and_projected(dev, diffusion):
    from diffusionremotesensing_amd import consistency, synthetic
    from diffusionremotesensing_amd.consistency import BandOperator, LRConsistency
    d, m = diffusion, diffusion.model
    assert d.mtf_nyquist == SAMPLE_GAINS
    lr = synthetic.tensor_uniform("mtf.lr", (3, 16, 16))

    def sample():
        return d.sample(2, m, lr, input_channels=3, noise_source=_src(40), sampling_steps=3)
    assert d.lr_consistency is None
    plain = sample()
    d.lr_consistency = LRConsistency(strength=0.0)
    try:
        assert bits_equal(sample(), plain)
        d.lr_consistency = LRConsistency(damping=0.0)
        projected = sample()
    finally:
        d.lr_consistency = None
    assert not bits_equal(projected, plain) and torch.isfinite(projected).all()
    op = LRConsistency().operator_for(d, (32, 32))
    assert isinstance(op, BandOperator) and len(op.operators) == 3
    y = lr.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
    free, kept = consistency.lr_rmse(plain, y, op), consistency.lr_rmse(projected, y, op)
    print(f"lr_rmse under the band operator: free chain {free.tolist()}, projected {kept.tolist()}, |projected| max "
          f"{float(projected.abs().max()):.3g}")
    assert float(free.min()) > 100 * float(kept.max())  # (the factor of the shared-operator test, against the free chain)


def test_evaluate_rows(dev, diffusion):
    from diffusionremotesensing_amd import consistency, hip_ops, synthetic
    from diffusionremotesensing_amd.consistency import LRConsistency
    d, m = diffusion, diffusion.model
    hr = synthetic.tensor_uniform("mtf.eval.hr", (2, 3, 32, 32))
    lr = synthetic.tensor_uniform("mtf.eval.lr", (2, 3, 16, 16))
    req = LRConsistency(damping=0.0)
    res = d.evaluate(m, [(lr, hr)], sampling_steps=3, noise_source=_src(55), lr_consistency=req)
    assert d.lr_consistency is None
    assert list(res) == ["model", "model_free", "bicubic", "per_image", "n"]
    assert set(res["model"]) == set(res["model_free"]) == set(res["bicubic"]) == {"psnr", "ssim", "sam", "ergas", "lr_rmse"}
    op = req.operator_for(d, (32, 32))
    y = lr.to(dev)
    d.lr_consistency = req
    try:
        x = d.sample(2, m, y, input_channels=3, noise_source=_src(55), sampling_steps=3)
    finally:
        d.lr_consistency = None
    want = {"model": consistency.lr_rmse(x.clamp(0, 1), y, op),
            "bicubic": consistency.lr_rmse(hip_ops.bicubic_upsample(y, 2).clamp(0, 1), y, op)}
    for name, v in want.items():
        assert res["per_image"][name]["lr_rmse"] == v.tolist(), name
    assert res["model"]["lr_rmse"] < res["model_free"]["lr_rmse"]


def test_tiler_projects_the_scene_with_a_band_operator(dev, diffusion):
    """A 48 x 64 scene (LR 24 x 32) of 32 x 32 tiles: the scene with `lr_consistency` is the plain scene of the same noise,
    projected as a whole with the scene-sized band operator and clamped, in both aggregation modes."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.consistency import LRConsistency
    d = diffusion
    img = 0.25 + 0.5 * synthetic.tensor_uniform("mtf.scene", (1, 3, 24, 32))
    tiler = split_aggregation_sampling(img.to(dev), 16, 8, 2, d, dev)

    def tile_noise(tile, i, shape):
        return torch.randn(shape, generator=torch.Generator().manual_seed(900 + 53 * tile + i))
    proj = MO.BandProjection(48, 64, 2, SAMPLE_GAINS, 0.0, lr_hw=(24, 32))
    plain = tiler.aggregation_sampling(noise_source=tile_noise, sampling_steps=3)
    got = tiler.aggregation_sampling(noise_source=tile_noise, sampling_steps=3, lr_consistency=LRConsistency(damping=0.0))
    assert tuple(got.shape) == (1, 3, 48, 64)
    want, bound = proj.project(plain.double().cpu().numpy(), img.double().numpy())
    err = np.abs(got.double().cpu().numpy() - np.clip(want, 0.0, 1.0))
    print(f"tiler: max |err| {err.max():.3e}, worst err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all() and not bits_equal(got, plain)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    per_step = tiler.aggregation_sampling(noise_source=_src(70), sampling_steps=3, aggregation="per_step")
    per_step_p = tiler.aggregation_sampling(noise_source=_src(70), sampling_steps=3, aggregation="per_step",
                                            lr_consistency=LRConsistency(damping=0.0))
    want, bound = proj.project(per_step.double().cpu().numpy(), img.double().numpy())
    assert (np.abs(per_step_p.double().cpu().numpy() - np.clip(want, 0.0, 1.0)) <= bound).all()


# ---------------------------------------------------------------------------------------------
# command lines
# ---------------------------------------------------------------------------------------------
_RUN = ["--image_size", "16", "--noise_steps", "10", "--epochs", "1", "--batch_size", "2", "--check_preds_epoch", "1", "--loss", "MSE",
        "--dataset_path", "synthetic_u16:8", "--bit_depth", "16", "--scene_size", "32", "--nodata", "0", "--magnification_factor", "2"]


def test_trainer_and_evaluate(dev, tmp_path, monkeypatch, capsys):
    """--Degradation_type MTF on the 16-bit entrance with windows, augmentation, no-data and noise: the run trains, writes
    MTF_NYQUIST into its snapshot and samples; `evaluate` takes the gains from the snapshot and scores under the band operator;
    a resume under other gains is refused."""
    import json
    import math
    from diffusionremotesensing_amd import evaluate
    from diffusionremotesensing_amd import train_diffusion_superres as T
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    mtf_run = _RUN + ["--model_name", "sr_mtf", "--data_range", "0,10000", "--augment", "d4", "--Degradation_type", "MTF"]
    T.main(mtf_run + ["--mtf_nyquist", "0.35,0.3,0.26", "--mtf_noise", "0.01"])
    out = capsys.readouterr().out
    assert "Running Val loss" in out and "Training snapshot saved" in out
    snapshot = torch.load(tmp_path / "models_run" / "sr_mtf" / "weights" / "snapshot.pt")
    assert snapshot["MTF_NYQUIST"] == [0.35, 0.3, 0.26] and "DATA_RANGE" in snapshot
    res = torch.load(tmp_path / "models_run" / "sr_mtf" / "results" / "superres_results.pt")
    assert tuple(res.shape) == (5, 3, 16, 16) and bool(torch.isfinite(res).all())
    scores = evaluate.main(_RUN + ["--model_name", "sr_mtf", "--n_images", "2", "--sampling_steps", "4", "--lr_consistency",
                                   "--out", str(tmp_path / "scores.json")])
    assert scores["n"] == 2 and {"lr_rmse", "valid_fraction"} <= set(scores["model"]) and "model_free" in scores
    assert all(math.isfinite(v) for v in scores["model"].values()), scores["model"]
    assert scores["model"]["lr_rmse"] < scores["model_free"]["lr_rmse"]
    assert json.load(open(tmp_path / "scores.json"))["args"]["Degradation_type"] == "MTF"
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --mtf_nyquist 0\.35,0\.3,0\.26, this run has 0\.3,0\.3,0\.3"):
        T.main(mtf_run + ["--mtf_nyquist", "0.3"])
    with pytest.raises(ValueError, match="this run has none"):
        T.main(_RUN + ["--model_name", "sr_mtf", "--data_range", "0,10000", "--Blur_radius", "0.5"])
