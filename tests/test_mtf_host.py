"""Host side of the sensor-MTF degradation (no device): the taps against their defining gain, the dense
operator against tests/mtf_oracle.py, `BandOperator`, the parsers and refusals, `LRConsistency` on an MTF diffusion, the
MTF_NYQUIST key of snapshots and train_state.pt, and the argument errors of the four new C entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import mtf_oracle as MO

FACTORS, GAINS = (2, 3, 4, 8), (0.05, 0.1, 0.2, 0.3, 0.4, 0.6)


@pytest.mark.parametrize("m", FACTORS)
def test_taps_have_their_nyquist_gain_and_are_symmetric(m):
    from diffusionremotesensing_amd import mtf
    for g in GAINS:
        k, L = mtf.gaussian_taps(g, m)
        want, want_L = MO.taps(g, m)
        assert L == want_L == int(np.ceil(3 * mtf.nyquist_sigma(g, m))) and k.shape == (2 * L + m,) and k.shape[0] <= mtf.MAX_TAPS
        assert np.array_equal(k, want) and np.array_equal(k, k.astype(np.float32).astype(np.float64))
        assert np.array_equal(k, k[::-1])  # symmetric about the LR pixel's centre
        assert abs(k.sum() - 1.0) <= 1e-7
        gain = MO.dtft_gain(k, m)
        print(f"m={m} g={g}: n={k.shape[0]} sigma={mtf.nyquist_sigma(g, m):.4f} gain {gain:.5f} ({100 * (gain / g - 1):+.2f} %)")
        assert abs(gain / g - 1.0) <= 0.02
    assert mtf.gaussian_taps(0.05, 8)[0].shape[0] == 46


def test_refused_factors_and_gains():
    from diffusionremotesensing_amd import mtf
    for m in (1, 9, 0, 2.0, True):
        with pytest.raises(ValueError, match="2 .. 8"):
            mtf.gaussian_taps(0.3, m)
    for g in (0.04, 0.61, 0.8, float("nan"), "0.3", True):
        with pytest.raises(ValueError, match="0.05 .. 0.6"):
            mtf.gaussian_taps(g, 2)


@pytest.mark.parametrize("H,W,m,g", [(24, 24, 2, 0.3), (20, 28, 4, 0.2), (70, 66, 3, 0.6), (8, 16, 8, 0.05), (64, 128, 2, 0.05)])
def test_dense_operator_is_the_oracles(H, W, m, g):
    from diffusionremotesensing_amd.consistency import SeparableOperator
    op = SeparableOperator.mtf((H, W), m, g)
    k, L = MO.taps(g, m)
    assert op.lr_shape == (H // m, W // m) and op.hr_shape == (H, W)  # not swapped
    assert np.array_equal(op.A_y, MO.dense(H, H // m, k, L, m)) and np.array_equal(op.A_x, MO.dense(W, W // m, k, L, m))
    for A in (op.A_y, op.A_x):
        assert np.abs(A.sum(axis=1) - k.sum()).max() <= 1e-12 and np.abs(A.sum(axis=1) - 1.0).max() <= 1e-7
    # the dense and the FIR form are one map
    x = np.random.default_rng(H + W).random((2, H, W))
    assert np.abs(op.apply(x) - MO.fir(x, k, k, L, L, m)).max() <= 1e-14
    cond = [np.linalg.cond(A) for A in (op.A_y, op.A_x)]
    assert max(cond) < 20
    op.factors(0.0)  # passes the 1e6 guard undamped
    lr = SeparableOperator.mtf((H, W), m, g, lr_hw=(H // m, W // m - 1 if W // m > 1 else 1))
    assert lr.lr_shape[1] == max(W // m - 1, 1)
    with pytest.raises(ValueError, match="does not fit"):
        SeparableOperator.mtf((H, W), m, g, lr_hw=(H // m + 1, W // m))
    with pytest.raises(ValueError, match="2 .. 8"):
        SeparableOperator.mtf((H, W), 1, g)


def test_band_operator():
    from diffusionremotesensing_amd import mtf
    from diffusionremotesensing_amd.consistency import BandOperator, LRConsistency, SeparableOperator
    gains = [0.35, 0.35, 0.34, 0.26, 0.35]
    b = BandOperator.mtf((20, 28), 2, gains)
    assert len(b.operators) == 3 and b.band_op == [0, 0, 1, 2, 0] and b.bands == 5  # equal gains share an operator
    assert b.hr_shape == (20, 28) and b.lr_shape == (10, 14)
    rows, L, band_op = mtf.band_taps(gains, 2)
    want_rows, want_L, want_op = MO.band_taps(gains, 2)
    assert np.array_equal(rows, want_rows) and L == want_L and band_op == want_op == b.band_op
    f = b.factors(0.01)
    assert f["D_y"].shape == (3, 10, 20) and f["D_x"].shape == (3, 14, 28) and f["U_y"].shape == (3, 20, 10)
    assert f["U_x"].shape == (3, 28, 14) and f["G"].shape == (3, 10, 14) and f["P_y"].shape == (3, 10, 10) and f["P_x"].shape == (3, 14, 14)
    assert np.array_equal(f["G"][1], b.operators[1].factors(0.01)["G"])
    A_y, A_x = b.matrices("cpu")
    assert tuple(A_y.shape) == (3, 10, 20) and tuple(A_x.shape) == (3, 14, 28) and A_y.dtype == torch.float32
    x = np.random.default_rng(3).random((2, 5, 20, 28))
    got = b.apply(x)
    for c, o in enumerate(b.band_op):  # the per-band loop
        assert np.array_equal(got[:, c], b.operators[o].apply(x[:, c]))
    k, L1 = MO.taps(0.26, 2)
    assert np.abs(got[:, 3] - MO.fir(x[:, 3], k, k, L1, L1, 2)).max() <= 1e-14
    with pytest.raises(ValueError, match="bands"):
        b.apply(x[:, :4])
    one = SeparableOperator.mtf((20, 28), 2, 0.3)
    for ops, idx, words in (([], [0], "1 .. 16"), ([one], [1], "outside"), ([one, one], [0], "bands"), ([one], [0] * 17, "bands"),
                            ([one, SeparableOperator.mtf((20, 24), 2, 0.3)], [0, 1], "differ in shape"), ([one], "ab", "index per band")):
        with pytest.raises(ValueError, match=words):
            BandOperator(ops, idx)
    assert LRConsistency(operator=b).operator is b  # accepted beside a SeparableOperator
    with pytest.raises(ValueError, match="takes"):
        LRConsistency(operator=b).operator_for(None, (24, 24))


def test_parsers():
    from diffusionremotesensing_amd import mtf
    assert mtf.parse_mtf_nyquist("0.3", 4) == (0.3,) * 4
    assert mtf.parse_mtf_nyquist("0.35,0.35,0.34,0.26", 4) == (0.35, 0.35, 0.34, 0.26)
    assert mtf.parse_mtf_nyquist(0.2, 2) == (0.2, 0.2) and mtf.parse_mtf_nyquist([0.2, 0.3], 2) == (0.2, 0.3)
    assert mtf.parse_mtf_noise("0,0.01,0.02", 3) == (0.0, 0.01, 0.02) and mtf.parse_mtf_noise("0.01", 2) == (0.01, 0.01)
    for text, bands, words in (("0.3,0.2", 3, r"--mtf_nyquist='0.3,0.2' names 2 values, the images have 3 bands"),
                               ("0.7", 3, "--mtf_nyquist=0.7 must be a number in 0.05 .. 0.6"), ("0.01", 1, "--mtf_nyquist=0.01"),
                               ("a,b", 2, "--mtf_nyquist='a,b': expected")):
        with pytest.raises(ValueError, match=words):
            mtf.parse_mtf_nyquist(text, bands)
    for text, bands, words in (("-0.1", 1, "--mtf_noise=-0.1 must be a finite number >= 0"), ("0.1,0.2", 3, "--mtf_noise='0.1,0.2' names 2"),
                               ("inf", 1, "--mtf_noise=inf"), ("x", 1, "--mtf_noise='x': expected")):
        with pytest.raises(ValueError, match=words):
            mtf.parse_mtf_noise(text, bands)


class _Model(nn.Linear):
    image_channels = 3


def _stub(tmp_path, model=None, **kw):
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    kw.setdefault("Degradation_type", "MTF")
    return Diffusion("cosine", model or _Model(3, 2), str(tmp_path / "run" / "snapshot.pt"), noise_steps=10, device="cpu", image_size=8,
                     magnification_factor=2, **kw)


def _train(d, **kw):
    d.train(lr=1e-3, epochs=1, check_preds_epoch=1, train_loader=[], val_loader=None, patience=5, loss="MSE", verbose=False, **kw)
    return d


def test_diffusion_attributes_and_refusals(tmp_path):
    d = _stub(tmp_path, mtf_nyquist="0.35,0.3,0.26", mtf_noise=0.01)
    assert d.mtf_nyquist == (0.35, 0.3, 0.26) and d.mtf_noise == (0.01, 0.01, 0.01)
    assert _stub(tmp_path, mtf_nyquist=0.3).mtf_nyquist == (0.3, 0.3, 0.3) and _stub(tmp_path, mtf_nyquist=0.3).mtf_noise is None
    assert _stub(tmp_path, model=nn.Linear(3, 2), mtf_nyquist=[0.3, 0.2]).mtf_nyquist == (0.3, 0.2)  # a model that names no band count
    plain = _stub(tmp_path, Degradation_type="DownBlur")
    assert plain.mtf_nyquist is None and plain.mtf_noise is None
    with pytest.raises(ValueError, match="needs mtf_nyquist"):
        _stub(tmp_path)
    with pytest.raises(ValueError, match="names 2 values, the images have 3 bands"):
        _stub(tmp_path, mtf_nyquist="0.3,0.2")
    with pytest.raises(ValueError, match="0.05 .. 0.6"):
        _stub(tmp_path, mtf_nyquist=0.8)
    with pytest.raises(ValueError, match="belong to Degradation_type='MTF'"):
        _stub(tmp_path, Degradation_type="DownBlur", mtf_nyquist=0.3)
    with pytest.raises(ValueError, match="belong to Degradation_type='MTF'"):
        _stub(tmp_path, Degradation_type="BSRGAN", mtf_noise=0.1)
    from diffusionremotesensing_amd.train_diffusion_superres import Diffusion
    with pytest.raises(ValueError, match="magnification_factor=1 must be an integer in 2 .. 8"):
        Diffusion("cosine", _Model(3, 2), str(tmp_path / "s.pt"), noise_steps=10, device="cpu", image_size=8, magnification_factor=1,
                  Degradation_type="MTF", mtf_nyquist=0.3)


def test_lr_consistency_on_an_mtf_diffusion(tmp_path):
    from diffusionremotesensing_amd import consistency
    from diffusionremotesensing_amd.consistency import BandOperator, LRConsistency
    d = _stub(tmp_path, mtf_nyquist="0.35,0.3,0.35")
    req = LRConsistency(damping=0.0)
    assert req.check_for(d) == (0.35, 0.3, 0.35)
    op = req.operator_for(d, (20, 28))
    assert isinstance(op, BandOperator) and op.band_op == [0, 1, 0] and op.lr_shape == (10, 14)
    assert req.operator_for(d, (20, 28), lr_hw=(9, 14)).lr_shape == (9, 14)
    k, L = MO.taps(0.3, 2)
    assert np.array_equal(op.operators[1].A_x, MO.dense(28, 14, k, L, 2))
    with pytest.raises(ValueError, match="blur_radius belongs to the DownBlur operator"):
        LRConsistency(blur_radius=0.5).check_for(d)
    # the chain's cache keys on the gains: another table, another operator
    seen = {}
    consistency._OPERATORS.clear()

    class _P:
        def projector(self, damping, device):
            return self
    try:
        orig = LRConsistency.operator_for
        LRConsistency.operator_for = lambda self, diffusion, size_hw, lr_hw=None: seen.setdefault(self.check_for(diffusion), _P())
        a = consistency.chain_projector(d, req, (8, 8), "cpu")
        assert consistency.chain_projector(d, req, (8, 8), "cpu") is a
        other = _stub(tmp_path, mtf_nyquist="0.35,0.3,0.3")
        assert consistency.chain_projector(other, req, (8, 8), "cpu") is not a
        assert set(consistency._OPERATORS) == {(8, 8, 2, (0.35, 0.3, 0.35)), (8, 8, 2, (0.35, 0.3, 0.3))}
    finally:
        LRConsistency.operator_for = orig
        consistency._OPERATORS.clear()


def test_mtf_nyquist_in_snapshot_and_resume_mismatch(tmp_path, monkeypatch):
    os.makedirs(tmp_path / "run")
    monkeypatch.setattr(torch.cuda, "get_rng_state", lambda device=None: torch.zeros(1, dtype=torch.uint8))
    snap, state = str(tmp_path / "run" / "snapshot.pt"), str(tmp_path / "run" / "train_state.pt")
    # a default run writes the files it always wrote: the reference's two keys
    _train(_stub(tmp_path, Degradation_type="DownBlur"), save_train_state=True)
    assert set(torch.load(snap)) == {"MODEL_STATE", "EPOCHS_RUN"} and "MTF_NYQUIST" not in torch.load(state)
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --mtf_nyquist none \(not an MTF run\), this run has 0\.3,0\.3,0\.3"):
        _stub(tmp_path, mtf_nyquist=0.3)
    os.remove(snap), os.remove(state)
    _train(_stub(tmp_path, mtf_nyquist="0.35,0.3,0.26"), save_train_state=True)
    for path in (snap, state):
        assert torch.load(path)["MTF_NYQUIST"] == [0.35, 0.3, 0.26]
    assert set(torch.load(snap)) == {"MODEL_STATE", "EPOCHS_RUN", "MTF_NYQUIST"}
    _train(_stub(tmp_path, mtf_nyquist=(0.35, 0.3, 0.26)), save_train_state=True)  # the same table: goes on
    with pytest.raises(ValueError, match=r"snapshot\.pt was written with --mtf_nyquist 0\.35,0\.3,0\.26, this run has 0\.35,0\.3,0\.25"):
        _stub(tmp_path, mtf_nyquist="0.35,0.3,0.25")
    with pytest.raises(ValueError, match="this run has none"):
        _stub(tmp_path, Degradation_type="DownBlur")
    ts = torch.load(state)  # train_state.pt alone disagrees
    ts["MTF_NYQUIST"] = [0.35, 0.3, 0.2]
    torch.save(ts, state)
    with pytest.raises(ValueError, match=r"train_state\.pt was written with --mtf_nyquist 0\.35,0\.3,0\.2,"):
        _train(_stub(tmp_path, mtf_nyquist="0.35,0.3,0.26"), save_train_state=True)


def test_feed_refusals_need_no_device():
    from diffusionremotesensing_amd.mtf import DeviceMTFFeed
    u8, u16 = torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 3, 8, 8), dtype=torch.uint16)
    f = DeviceMTFFeed(u16, 2, "0.3,0.2,0.3", noise=0.01, nodata=7, batch_size=2)
    assert f.operator.band_op == [0, 1, 0] and f.nyquist == (0.3, 0.2, 0.3) and f.noise == (0.01,) * 3 and len(f) == 1 and f.nodata == 7
    assert f.taps.shape[0] == 2 and f.taps.shape[1] == 2 * f.left + 2
    with pytest.raises(ValueError, match="nodata belongs to a uint16 cache"):
        DeviceMTFFeed(u8, 2, 0.3, nodata=0)
    with pytest.raises(ValueError, match="2 .. 8"):
        DeviceMTFFeed(u8, 1, 0.3)
    with pytest.raises(ValueError, match="names 2 values"):
        DeviceMTFFeed(u8, 2, "0.3,0.2")
    with pytest.raises(ValueError, match="square windows"):
        DeviceMTFFeed(torch.zeros((2, 3, 8, 12), dtype=torch.uint8), 2, 0.3)
    with pytest.raises(RuntimeError, match="uint8 or torch.uint16"):
        DeviceMTFFeed(torch.zeros((2, 3, 8, 8)), 2, 0.3)
    with pytest.raises(RuntimeError, match="ROCm"):
        f.batch(np.zeros((1, 4), dtype=np.int32))


def test_argument_validation_without_gpu():
    """The new entries refuse their arguments before they touch a device (fake, never dereferenced pointers)."""
    from diffusionremotesensing_amd import _lib
    lib = _lib.load()
    P = C.c_void_p
    x, out, taps = P(1 << 20), P(1 << 24), P(1 << 12)

    def fir(**kw):
        a = dict(x=x, ty=taps, tx=taps, band_op=None, n_ops=1, ny=8, nx=8, Ly=3, Lx=3, m=2, noise=None, sigma=None, clamp=0, out=out,
                 n=1, c=3, H=16, W=16, h=8, w=8)
        a.update(kw)
        return lib.drs_fir_decimate(a["x"], a["ty"], a["tx"], a["band_op"], a["n_ops"], a["ny"], a["nx"], a["Ly"], a["Lx"], a["m"],
                                    a["noise"], a["sigma"], a["clamp"], a["out"], a["n"], a["c"], a["H"], a["W"], a["h"], a["w"], None)

    def refused(status, words, **kw):
        assert fir(**kw) == status, kw
        assert words in lib.drs_last_error(), (kw, lib.drs_last_error())
    for name in ("x", "ty", "tx", "out"):
        refused(1, b"null pointer", **{name: None})
    refused(1, b"go together", noise=P(1 << 16))
    refused(1, b"go together", sigma=P(1 << 16))
    refused(1, b"overlap", out=P((1 << 20) + 64))
    refused(1, b"overlap", out=P((1 << 20) - 64))
    table = (C.c_int32 * 3)
    for kw, words in (({"c": 17}, b"at most 16"), ({"n_ops": 0}, b"n_ops=0"), ({"n_ops": 4}, b"n_ops=4"),
                      ({"n_ops": 2, "band_op": table(0, 2, 1)}, b"band_op[1]=2"), ({"band_op": table(0, -1, 0)}, b"band_op[1]=-1"),
                      ({"m": 0}, b"m=0"), ({"m": 9}, b"m=9"), ({"ny": 0}, b"ntaps_y=0"), ({"nx": 65}, b"ntaps_x=65"),
                      ({"Ly": 8}, b"Ly=8"), ({"Lx": -1}, b"Lx=-1"), ({"h": 9}, b"h m"), ({"w": 9}, b"w m"), ({"n": 0}, b"extent"),
                      ({"h": 0}, b"extent"), ({"H": 1 << 16, "W": 1 << 15, "h": 1, "w": 1}, b"2^31")):
        refused(2, words, **kw)
    # m = 1 is the entry's (a general FIR); only the Python layer refuses it: past the checks this would launch, so not called
    ws = P(1 << 28)

    def sep(entry, **kw):
        a = dict(n=1, c=3, H=8, W=8, h=4, w=4, band_op=None, n_ops=1, bytes=1 << 20)
        a.update(kw)
        tail = (a["n"], a["c"], a["H"], a["W"], a["h"], a["w"], a["band_op"], a["n_ops"], ws, a["bytes"], None)
        if entry == "apply":
            return lib.drs_sep_apply_bands(x, taps, taps, out, *tail)
        if entry == "project":
            return lib.drs_sep_project_bands(x, x, taps, taps, taps, taps, taps, 1.0, out, *tail)
        return lib.drs_sep_project_eps_bands(out, x, x, taps, 10, x, taps, taps, taps, taps, taps, 1.0, *tail)
    for entry in ("apply", "project", "project_eps"):
        name = f"sep_{entry}_bands".encode()
        for kw, status, words in (({"n_ops": 0}, 2, b"n_ops=0"), ({"n_ops": 4}, 2, b"n_ops=4"), ({"c": 17}, 2, b"at most 16"),
                                  ({"n_ops": 2, "band_op": table(0, 1, 2)}, 2, b"band_op[2]=2"), ({"bytes": 8}, 4, b"workspace")):
            assert sep(entry, **kw) == status, (entry, kw)
            assert name in lib.drs_last_error() and words in lib.drs_last_error(), (entry, kw, lib.drs_last_error())
    assert lib.drs_sep_apply_bands(None, taps, taps, out, 1, 3, 8, 8, 4, 4, None, 1, ws, 1 << 20, None) == 1
    assert b"sep_apply_bands: null pointer" in lib.drs_last_error()
    assert lib.drs_abi_version() == 8


def test_hip_ops_refusals_need_no_device():
    from diffusionremotesensing_amd import hip_ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm"):
        hip_ops.fir_decimate(x, torch.zeros(8), torch.zeros(8), 3, 2)
    assert hip_ops._band_table("op", None, 2, 3) is None
    assert list(hip_ops._band_table("op", [0, 1, 1], 2, 3)) == [0, 1, 1]
    for band_op, n_ops in (([0, 1], 2), ([0, 1, 2], 2), ([0, -1, 0], 2), (None, 4), (None, 0)):
        with pytest.raises(RuntimeError, match="op:"):
            hip_ops._band_table("op", band_op, n_ops, 3)


def test_trainer_flags_and_refusals(capsys):
    from diffusionremotesensing_amd import train_diffusion_superres as sr
    base = ["--magnification_factor", "2"]
    mtf = base + ["--Degradation_type", "MTF", "--mtf_nyquist", "0.3"]
    args = sr.parse_train_args(base)
    assert args.mtf_nyquist is None and args.mtf_noise is None
    args = sr.parse_train_args(base + ["--Degradation_type", "MTF", "--mtf_nyquist", "0.35,0.3,0.26", "--mtf_noise", "0.01",
                                       "--dataset_path", "synthetic_u8:8"])
    assert args.mtf_nyquist == (0.35, 0.3, 0.26) and args.mtf_noise == (0.01, 0.01, 0.01)
    args = sr.parse_train_args(mtf + ["--bit_depth", "16", "--nodata", "777", "--dataset_path", "synthetic_u16:8"])  # beside downblur
    assert args.mtf_nyquist == (0.3, 0.3, 0.3) and args.nodata == 777
    capsys.readouterr()
    for argv, words in (
            (base + ["--mtf_nyquist", "0.3"], "--mtf_nyquist belongs to --Degradation_type MTF"),
            (base + ["--mtf_noise", "0.01"], "--mtf_noise belongs to --Degradation_type MTF"),
            (base + ["--Degradation_type", "MTF"], "--Degradation_type MTF needs --mtf_nyquist"),
            (["--magnification_factor", "1", "--Degradation_type", "MTF", "--mtf_nyquist", "0.3"], "--magnification_factor 1 must lie in 2 .. 8"),
            (["--magnification_factor", "9", "--Degradation_type", "MTF", "--mtf_nyquist", "0.3"], "--magnification_factor 9 must lie in 2 .. 8"),
            (mtf + ["--dataset_path", "synthetic:8"], "--dataset_path 'synthetic:8': the float DataLoader path"),
            (mtf + ["--Blur_radius", "0.5"], "--Blur_radius belongs to the DownBlur degradations"),
            (mtf + ["--nodata", "5"], "--nodata with --Degradation_type MTF needs --bit_depth 16"),
            (mtf + ["--mtf_nyquist", "0.3,0.2"], "names 2 values, the images have 3 bands"),
            (mtf + ["--mtf_nyquist", "0.7"], "--mtf_nyquist=0.7 must be a number in 0.05 .. 0.6"),
            (mtf + ["--mtf_noise", "-1"], "--mtf_noise=-1.0 must be a finite number >= 0")):
        with pytest.raises(SystemExit):
            sr.parse_train_args(argv)
        assert words in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):  # registered without a --help entry: the trainer's help text is recorded
        sr.parse_train_args(["--help"])
    assert "mtf" not in capsys.readouterr().out
    args = sr.parse_train_args(mtf)  # `launch` refuses the same before it touches a device
    args.Blur_radius = "0.5"
    with pytest.raises(ValueError, match="--Blur_radius belongs"):
        sr.launch(args)


def test_evaluate_and_tiler_flags(tmp_path):
    from diffusionremotesensing_amd import Aggregation_Sampling as A
    from diffusionremotesensing_amd import evaluate, mtf
    p = evaluate.cli_arg_parser("superres")
    assert "--mtf_nyquist" in p.format_help() and "--mtf_noise" not in p.format_help()
    assert p.parse_args(["--mtf_nyquist", "0.3,0.2,0.3"]).mtf_nyquist == "0.3,0.2,0.3" and p.parse_args([]).mtf_nyquist is None
    assert "--mtf_nyquist" not in evaluate.cli_arg_parser("sar_to_ndvi").format_help()
    t = A.build_arg_parser()
    assert "--mtf_nyquist" in t.format_help() and t.parse_args(["--mtf_nyquist", "0.3"]).mtf_nyquist == "0.3"
    # the default is the snapshot's table; a snapshot without the key and no flag: not an MTF run
    plain, trained = str(tmp_path / "plain.pt"), str(tmp_path / "mtf.pt")
    torch.save({"MODEL_STATE": {}, "EPOCHS_RUN": 1}, plain)
    torch.save({"MODEL_STATE": {}, "EPOCHS_RUN": 1, "MTF_NYQUIST": [0.35, 0.3, 0.26]}, trained)
    none, flag = p.parse_args([]), p.parse_args(["--mtf_nyquist", "0.2"])
    assert mtf.resolve_nyquist(none, plain, 3) is None and mtf.resolve_nyquist(none, str(tmp_path / "missing.pt"), 3) is None
    assert mtf.resolve_nyquist(none, trained, 3) == (0.35, 0.3, 0.26)
    assert mtf.resolve_nyquist(flag, trained, 3) == (0.2, 0.2, 0.2) and mtf.resolve_nyquist(flag, plain, 3) == (0.2, 0.2, 0.2)
    with pytest.raises(ValueError, match="the images have 4 bands"):
        mtf.resolve_nyquist(none, trained, 4)
