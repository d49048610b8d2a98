"""LR-consistent sampling on the device: the three launching entries of csrc/consistency.hip against
the float64 oracle within its bound (tests/consistency_oracle.py), repeatability, the identity at strength 0, the agreement of
the eps form with the x0 form, projected reverse chains against the oracle's chain, `Diffusion.sample` with the attribute off
and at strength 0, and the tiler's projection of the finished scene."""
import numpy as np
import pytest
import torch

import consistency_oracle as CO
from guard import bits_equal
from oracle import diffusion_oracle as D

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 24, 24, 2), (1, 1, 20, 28, 4), (3, 16, 32, 32, 2), (1, 3, 72, 64, 2), (1, 3, 256, 256, 2)]
SETTINGS = [(0.5, 0.0), (0.5, 0.01), (1.0, 0.01)]  # (blur radius, damping): the exact pseudo-inverse only where it is harmless
T = 50
LEVELS = [1, 7, T // 2, T - 1]
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _schedule():
    return D.schedule("cosine", T)


def _case(shape, radius, damping):
    """Inputs (fp32 tensors) and the oracle's results of one (shape, operator), computed once and shared."""
    key = (shape, radius, damping)
    if key in _CASES:
        return _CASES[key]
    from diffusionremotesensing_amd.consistency import SeparableOperator
    B, Cn, H, W, m = shape
    op = SeparableOperator.downblur((H, W), m, radius)
    A_y, A_x = CO.downblur_matrices(H, W, m, radius)
    proj = CO.Projection(A_y, A_x, damping)
    g = torch.Generator().manual_seed(7 + H + 3 * W + Cn)
    yy, xx = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, indexing="ij")
    truth = (0.5 + 0.3 * torch.sin(6.0 * xx + 1.0) * torch.cos(5.0 * yy))[None, None] + 0.05 * torch.randn((B, Cn, H, W), generator=g)
    x0 = (truth + 0.1 * torch.randn((B, Cn, H, W), generator=g)).float()
    y = torch.from_numpy(proj.degrade(truth.double().numpy())).float() + 0.01 * torch.randn((B, Cn) + op.lr_shape, generator=g)
    eps = torch.randn((B, Cn, H, W), generator=g)
    t = torch.tensor([LEVELS[(i + H) % len(LEVELS)] for i in range(B)])
    ah = _schedule()[1]
    a, s = ah[t].double().sqrt()[:, None, None, None], (1.0 - ah[t].double()).sqrt()[:, None, None, None]
    x = (a * x0.double() + s * eps.double()).float()  # the state whose implied x0 is (about) x0
    n = {k: v.double().numpy() for k, v in (("x0", x0), ("y", y), ("eps", eps), ("x", x))}
    case = {"op": op, "proj": proj, "x0": x0, "y": y, "eps": eps, "x": x, "t": t, "ah": ah,
            "degrade": (proj.degrade(n["x0"]), proj.gamma * proj.degrade_abs(n["x0"])),
            "project": proj.project(n["x0"], n["y"]),
            "project_eps": proj.project_eps(n["eps"], n["x"], ah[t].double().numpy(), n["y"])}
    _CASES[key] = case
    return case


def _within(got, want_bound, what):
    want, bound = want_bound
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| {err.max():.3e}, max bound {bound.max():.3e}, worst err / bound {ratio:.3e}")
    assert np.isfinite(err).all() and ratio <= 1.0, what


@pytest.mark.parametrize("radius,damping", SETTINGS, ids=[f"r{r}-d{d}" for r, d in SETTINGS])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_entries_vs_float64_oracle(dev, shape, radius, damping):
    from diffusionremotesensing_amd import consistency, hip_ops
    c = _case(shape, radius, damping)
    what = f"{shape} radius {radius} damping {damping}"
    projector = c["op"].projector(damping, dev)
    x0, y, eps, x, t, ah = (c[k].to(dev) for k in ("x0", "y", "eps", "x", "t", "ah"))
    lr = consistency.degrade(x0, c["op"])
    _within(lr, c["degrade"], f"degrade {what}")
    assert bits_equal(lr, consistency.degrade(x0, c["op"]))
    rm = consistency.lr_rmse(x0, y, c["op"]).double().cpu().numpy()
    want_rm = np.sqrt(((c["degrade"][0] - c["y"].double().numpy()) ** 2).mean(axis=(1, 2, 3)))
    assert np.allclose(rm, want_rm, rtol=1e-4, atol=1e-7)
    # the x0 form
    p = consistency.project(x0, y, projector)
    _within(p, c["project"], f"project {what}")
    assert bits_equal(p, consistency.project(x0, y, projector))  # two calls, the same bits
    assert bits_equal(consistency.project(x0, y, projector, strength=0.0), x0)
    in_place = x0.clone()
    assert consistency.project(in_place, y, projector, out=in_place) is in_place and bits_equal(in_place, p)
    # the in-chain form
    yt = projector.prepare(y)
    e1 = hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector)
    _within(e1, c["project_eps"], f"project_eps {what}")
    assert bits_equal(e1, hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector))
    assert bits_equal(hip_ops.lr_consistent_eps_(eps.clone(), x, t, ah, yt, projector, 0.0), eps)
    # the two forms agree: the x0 the corrected eps implies is the projection of the x0 the given eps implies
    a, s = (v.double().cpu()[:, None, None, None] for v in (ah[t].double().sqrt(), (1.0 - ah[t].double()).sqrt()))
    x0_in = ((c["x"].double() - s * c["eps"].double()) / a).float()
    from_x0 = consistency.project(x0_in.to(dev), y, projector).double().cpu()
    from_eps = (c["x"].double() - s * e1.double().cpu()) / a
    n_in = x0_in.double().numpy()
    bound = c["proj"].project(n_in, c["y"].double().numpy())[1] + (s / a).numpy() * c["project_eps"][1] \
        + 2.0 ** -24 * (np.abs(n_in) + c["proj"].correction_abs(np.abs(n_in), 0.0))  # (x0_in was rounded to fp32)
    ratio = float(((from_x0 - from_eps).abs().numpy() / bound).max())
    print(f"eps form vs x0 form {what}: worst |diff| / bound {ratio:.3e}")
    assert ratio <= 1.0
    if damping == 0.0:  # the undamped projection lands on the observation
        resid = np.abs(c["proj"].degrade(p.double().cpu().numpy()) - c["y"].double().numpy())
        assert (resid <= c["proj"].degrade_abs(c["project"][1])).all(), resid.max()


def test_a_level_outside_the_table_gives_nan(dev):
    from diffusionremotesensing_amd import hip_ops
    c = _case(SHAPES[0], 0.5, 0.01)
    projector = c["op"].projector(0.01, dev)
    eps, x, ah, y = (c[k].to(dev) for k in ("eps", "x", "ah", "y"))
    out = hip_ops.lr_consistent_eps_(eps.clone(), x, torch.tensor([T, 7], device=dev), ah, projector.prepare(y), projector)
    assert torch.isnan(out[0]).all() and torch.isfinite(out[1]).all()


# ---------------------------------------------------------------------------------------------
# projected chains
# ---------------------------------------------------------------------------------------------
class _Schedule:
    Degradation_type, magnification_factor, blur_radius = "DownBlur", 2, 0.5

    def __init__(self, n_steps, dev, request):
        self.noise_steps, self.device, self.lr_consistency = n_steps, dev, request
        self.tables = D.schedule("cosine", n_steps)
        self.alpha, self.alpha_hat, self.beta = (v.to(dev) for v in self.tables)


class _Engine:
    def check_faults(self):
        pass


CHAINS = {"ddim4": (50, 4), "ancestral6": (7, None)}


@pytest.mark.parametrize("kind", list(CHAINS))
def test_projected_chain_vs_float64_oracle(dev, kind):
    """Scripted predictions (a fixed eps per level), radius 0.5, damping 0: the fp32 chain stays within the oracle chain's
    running bound (per plane, in the Frobenius norm), and its un-clamped result maps to the observation within the bound of its last move."""
    from diffusionremotesensing_amd import sampling
    from diffusionremotesensing_amd.consistency import LRConsistency
    n_steps, S = CHAINS[kind]
    shape = (2, 3, 24, 24)
    sch = _Schedule(n_steps, dev, LRConsistency(damping=0.0))
    levels = sampling.chain_levels(n_steps, S)
    assert len(levels) == (4 if S else 6)
    g = torch.Generator().manual_seed(11)
    scripted = {t: torch.randn(shape, generator=g) for t in levels}
    noise = {t: torch.randn(shape, generator=g) for t in levels + [n_steps]}
    y = 0.2 + 0.6 * torch.rand((2, 3, 12, 12), generator=g)
    order = iter(levels)
    got = sampling.sample_chain(sch, _Engine(), shape, lambda e, x, t, first: scripted[next(order)].to(dev), table_rows=2,
                                noise_source=lambda i, shp: noise[i], sampling_steps=S, lr_img=y)
    proj = CO.Projection(*CO.downblur_matrices(24, 24, 2, 0.5), 0.0)
    alpha, ah, beta = (v.double().numpy() for v in sch.tables)
    want, E, resid_bound = CO.chain(proj, y.double().numpy(), ah, levels, lambda t: scripted[t].double().numpy(),
                                    lambda t: noise[t].double().numpy(), noise[n_steps].double().numpy(), ancestral=S is None,
                                    alpha=alpha, beta=beta)
    got = got.double().cpu().numpy()
    err = np.sqrt(((got - want) ** 2).sum(axis=(-2, -1), keepdims=True))  # per plane, the norm the running bound is kept in
    print(f"{kind}: max |err| {np.abs(got - want).max():.3e}, worst plane norm {err.max():.3e}, worst norm / bound {(err / E).max():.3e}")
    assert (err <= E).all()
    resid = np.abs(proj.degrade(got) - y.double().numpy())
    print(f"{kind}: max |A x - y| {resid.max():.3e}, worst / bound {(resid / resid_bound).max():.3e}")
    assert (resid <= resid_bound).all()


# ---------------------------------------------------------------------------------------------
# Diffusion.sample and the tiler
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def diffusion(dev, seeded_sd):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    m = Residual_Attention_UNet_superres(3, 3, dev)
    m.load_state_dict(seeded_sd)
    m = m.to(dev).eval()
    return Diffusion("cosine", m, "/nonexistent/snapshot.pt", noise_steps=50, device=dev, magnification_factor=2, image_size=32,
                     Degradation_type="DownBlur")


def _src(seed):
    return lambda i, shape: torch.randn(shape, generator=torch.Generator().manual_seed(seed + i))


def test_sample_with_the_attribute_off_and_at_strength_zero(dev, diffusion):
    from diffusionremotesensing_amd import consistency, synthetic
    from diffusionremotesensing_amd.consistency import LRConsistency
    d, m = diffusion, diffusion.model
    lr = synthetic.tensor_uniform("consistency.lr", (3, 16, 16))

    def sample():
        return d.sample(2, m, lr, input_channels=3, noise_source=_src(40), sampling_steps=3)
    assert d.lr_consistency is None
    plain = sample()
    del d.lr_consistency  # a Diffusion from before the attribute: the chain that has always run
    try:
        assert bits_equal(sample(), plain)
    finally:
        d.lr_consistency = None
    d.lr_consistency = LRConsistency(strength=0.0)
    try:
        assert bits_equal(sample(), plain)
        d.lr_consistency = LRConsistency(damping=0.0)
        projected = sample()
    finally:
        d.lr_consistency = None
    assert not bits_equal(projected, plain) and torch.isfinite(projected).all()
    op = LRConsistency().operator_for(d, (32, 32))
    y = lr.to(dev).unsqueeze(0).expand(2, -1, -1, -1).contiguous()
    # the plain sample of seeded (untrained) weights is nowhere near its LR image; the projected one is, to fp32 rounding of its
    # own magnitude (the last DDIM move returns the projected x0 itself)
    free, kept = consistency.lr_rmse(plain, y, op), consistency.lr_rmse(projected, y, op)
    print(f"lr_rmse: plain {free.tolist()}, projected {kept.tolist()}, |projected| max {float(projected.abs().max()):.3g}")
    assert float(kept.max()) <= 2.0 ** -16 * max(1.0, float(projected.abs().max())) and float(free.min()) > 100 * float(kept.max())


def test_tiler_projects_the_finished_scene(dev, diffusion):
    """A 48 x 40 scene (LR 24 x 20) of 32 x 32 tiles: the scene with `lr_consistency` is the plain scene of the same noise,
    projected as a whole and clamped - in both aggregation modes the projection is the tiler's last step but the clamp."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.Aggregation_Sampling import split_aggregation_sampling
    from diffusionremotesensing_amd.consistency import LRConsistency
    d = diffusion
    img = 0.25 + 0.5 * synthetic.tensor_uniform("consistency.scene", (1, 3, 24, 20))
    tiler = split_aggregation_sampling(img.to(dev), 16, 8, 2, d, dev)

    def tile_noise(tile, i, shape):
        return torch.randn(shape, generator=torch.Generator().manual_seed(900 + 53 * tile + i))
    plain = tiler.aggregation_sampling(noise_source=tile_noise, sampling_steps=3)
    got = tiler.aggregation_sampling(noise_source=tile_noise, sampling_steps=3, lr_consistency=LRConsistency(damping=0.0))
    assert tuple(got.shape) == (1, 3, 48, 40)
    proj = CO.Projection(*CO.downblur_matrices(48, 40, 2, 0.5, lr_hw=(24, 20)), 0.0)
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


def test_evaluate_rows(dev, diffusion):
    """`evaluate(lr_consistency=)`: the `model` row is the projected chain, `model_free` the plain chain of the same noise - with a
    `noise_source` and with torch's generators - and `lr_rmse` is `consistency.lr_rmse` of the clamped estimates; without the
    request the result has the keys it had."""
    from diffusionremotesensing_amd import consistency, hip_ops, synthetic
    from diffusionremotesensing_amd.consistency import LRConsistency
    d, m = diffusion, diffusion.model
    hr = synthetic.tensor_uniform("consistency.eval.hr", (2, 3, 32, 32))
    lr = synthetic.tensor_uniform("consistency.eval.lr", (2, 3, 16, 16))
    loader = [(lr, hr)]
    plain = d.evaluate(m, loader, sampling_steps=3, noise_source=_src(55))
    assert set(plain) == {"model", "bicubic", "per_image", "n"} and set(plain["model"]) == {"psnr", "ssim", "sam", "ergas"}
    req = LRConsistency(damping=0.0)
    res = d.evaluate(m, loader, sampling_steps=3, noise_source=_src(55), lr_consistency=req)
    assert d.lr_consistency is None  # put back
    assert list(res) == ["model", "model_free", "bicubic", "per_image", "n"]
    assert set(res["model"]) == set(res["model_free"]) == set(res["bicubic"]) == {"psnr", "ssim", "sam", "ergas", "lr_rmse"}
    for k in ("psnr", "ssim", "sam", "ergas"):  # the free chain is the chain of an evaluation without the request
        assert res["per_image"]["model_free"][k] == plain["per_image"]["model"][k], k
        assert res["per_image"]["bicubic"][k] == plain["per_image"]["bicubic"][k], k
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
    # without a noise source both chains draw from torch's generators, put back in between: the same x_T
    torch.manual_seed(5)
    drawn = d.evaluate(m, loader, sampling_steps=3, lr_consistency=req, baseline=False)
    torch.manual_seed(5)
    free = d.evaluate(m, loader, sampling_steps=3, baseline=False)
    assert drawn["per_image"]["model_free"]["psnr"] == free["per_image"]["model"]["psnr"]
    assert list(drawn) == ["model", "model_free", "per_image", "n"]
