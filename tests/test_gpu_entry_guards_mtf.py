"""The four entries of the sensor-MTF degradation - drs_fir_decimate (csrc/mtf.hip) and the per-band drs_sep_*_bands
(csrc/consistency.hip) - between guard bands at the three pointer phases of tests/guard.py, run through
`test_gpu_guard.guarded_runs` - so that they count for that module's `test_every_entry_point_that_launches_is_guarded`, which
walks `_lib.SIGNATURES` and runs after this file (files run in name order; on its own that test does not know these entries).

Every mode must give the bits of the normal call: a pointer off a 16-byte boundary makes a lane load its four consecutive
elements one by one instead of at once, and the same values reach the same multiply-add in the same order.  At (2, 3, 24, 24)
the aligned FIR call takes the 16-byte loads; at (1, 2, 70, 66, 3) W % 4 != 0 leaves it the element-wise loads whatever the
pointers are; (1, 3, 136, 136, 2) has several tiles per axis with a ragged last one."""
import types

import pytest
import torch

import test_gpu_guard as G
import test_gpu_mtf as GM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("shape,gains", [GM.FIR_CASES[0], GM.FIR_CASES[3], GM.FIR_CASES[6]], ids=lambda v: str(v))
def test_fir_decimate_between_guards(monkeypatch, dev, shape, gains):
    from diffusionremotesensing_amd import hip_ops
    c = GM._fir_case(shape, gains)

    def oracle(res):
        GM._within(res["lr"], c["plain"], "fir_decimate")
        GM._within(res["noisy"], c["noisy"], "fir_decimate + noise + clamp")

    def fn(put):
        x, rows_y, rows_x = put(c["x"].to(dev)), put(c["rows"].to(dev)), put(c["rows"].to(dev))
        return {"lr": hip_ops.fir_decimate(x, rows_y, rows_x, c["L"], c["m"], band_op=c["band_op"]),
                "noisy": hip_ops.fir_decimate(x, rows_y, rows_x, c["L"], c["m"], band_op=c["band_op"], noise=put(c["z"].to(dev)),
                                              sigma=put(c["sigma"].to(dev)), clamp=True),
                "x untouched": x}
    G.guarded_runs(monkeypatch, dev, "drs_fir_decimate", fn, oracle, case=str(shape))


def _guarded_projector(projector, put):
    names = ("D_y", "D_x", "U_y", "U_x", "G", "Pt_y", "Pt_x")
    return types.SimpleNamespace(**{k: put(getattr(projector, k)) for k in names}, band_op=projector.band_op)


@pytest.mark.parametrize("shape,gains,damping", [GM.PROJ_CASES[0], GM.PROJ_CASES[3]], ids=lambda v: str(v))
def test_sep_band_entries_between_guards(monkeypatch, dev, shape, gains, damping):
    from diffusionremotesensing_amd import hip_ops
    c = GM._proj_case(shape, gains, damping)
    projector = c["op"].projector(damping, dev)
    A_y, A_x = c["op"].matrices(dev)
    band_op = c["op"].band_op

    def apply(put):
        return {"lr": hip_ops.sep_apply(put(c["x0"].to(dev)), put(A_y), put(A_x), band_op=band_op)}
    G.guarded_runs(monkeypatch, dev, "drs_sep_apply_bands", apply, lambda res: GM._within(res["lr"], c["degrade"], "degrade"),
                   setup=hip_ops._SEP_WS.clear, case=str(shape))

    def project(put):
        p = _guarded_projector(projector, put)
        x0 = put(c["x0"].to(dev))
        yt = hip_ops.sep_apply(put(c["y"].to(dev)), p.Pt_y, p.Pt_x, band_op=band_op)
        out = hip_ops.sep_project(x0, yt, p, 1.0)
        in_place = put(c["x0"].to(dev))
        hip_ops.sep_project(in_place, yt, p, 1.0, out=in_place)
        return {"yt": yt, "out": out, "in place": in_place, "x0 untouched": x0, "strength 0": hip_ops.sep_project(x0, yt, p, 0.0)}
    G.guarded_runs(monkeypatch, dev, "drs_sep_project_bands", project, lambda res: GM._within(res["out"], c["project"], "project"),
                   setup=hip_ops._SEP_WS.clear, case=str(shape))

    def project_eps(put):
        p = _guarded_projector(projector, put)
        x, t, ah = (put(c[k].to(dev)) for k in ("x", "t", "ah"))
        yt = hip_ops.sep_apply(put(c["y"].to(dev)), p.Pt_y, p.Pt_x, band_op=band_op)
        eps = hip_ops.lr_consistent_eps_(put(c["eps"].to(dev)), x, t, ah, yt, p, 1.0)
        return {"eps": eps, "x untouched": x, "strength 0": hip_ops.lr_consistent_eps_(put(c["eps"].to(dev)), x, t, ah, yt, p, 0.0)}
    G.guarded_runs(monkeypatch, dev, "drs_sep_project_eps_bands", project_eps,
                   lambda res: GM._within(res["eps"], c["project_eps"], "project_eps"), setup=hip_ops._SEP_WS.clear, case=str(shape))
