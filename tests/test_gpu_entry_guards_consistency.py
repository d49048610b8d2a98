"""The entry points of csrc/consistency.hip between guard bands at the three pointer phases of tests/guard.py, run through
`test_gpu_guard.guarded_runs` - so that they count for that module's `test_every_entry_point_that_launches_is_guarded`, which
walks `_lib.SIGNATURES` and runs after this file (files run in name order; on its own that test does not know these entries).
`drs_sep_workspace_bytes` is recorded on the way: every wrapper asks it for the size of the workspace, which is dropped before
each run so that the block allocates it.

Every mode must give the bits of the normal call: a pointer off a 16-byte boundary makes a lane load its four consecutive
operands one by one instead of at once, and the same values reach the same multiply-add in the same order.  At (2, 3, 24, 24)
the aligned call takes the 16-byte loads in every product; at (1, 1, 20, 28), x4 - an LR image of 7 x 5 - the short rows leave
three of the four products the element-wise loads whatever the pointers are."""
import types

import pytest
import torch

import test_gpu_consistency as GC
import test_gpu_guard as G

pytestmark = pytest.mark.gpu

CASES = [(GC.SHAPES[0], 0.5, 0.01), (GC.SHAPES[1], 0.5, 0.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _guarded_projector(projector, put):
    """The projector's tensors as guarded copies: what the wrappers read them from."""
    names = ("D_y", "D_x", "U_y", "U_x", "G", "Pt_y", "Pt_x")
    return types.SimpleNamespace(**{k: put(getattr(projector, k)) for k in names})


@pytest.mark.parametrize("shape,radius,damping", CASES, ids=[str(c[0]) for c in CASES])
def test_sep_entries_between_guards(monkeypatch, dev, shape, radius, damping):
    from diffusionremotesensing_amd import hip_ops
    c = GC._case(shape, radius, damping)
    projector = c["op"].projector(damping, dev)
    A_y, A_x = c["op"].matrices(dev)

    def apply(put):
        return {"lr": hip_ops.sep_apply(put(c["x0"].to(dev)), put(A_y), put(A_x))}
    G.guarded_runs(monkeypatch, dev, "drs_sep_apply", apply, lambda res: GC._within(res["lr"], c["degrade"], "degrade"),
                   setup=hip_ops._SEP_WS.clear, case=str(shape))

    def project(put):
        p = _guarded_projector(projector, put)
        x0 = put(c["x0"].to(dev))
        yt = hip_ops.sep_apply(put(c["y"].to(dev)), p.Pt_y, p.Pt_x)
        out = hip_ops.sep_project(x0, yt, p, 1.0)
        in_place = put(c["x0"].to(dev))
        hip_ops.sep_project(in_place, yt, p, 1.0, out=in_place)
        return {"yt": yt, "out": out, "in place": in_place, "x0 untouched": x0,
                "strength 0": hip_ops.sep_project(x0, yt, p, 0.0)}
    G.guarded_runs(monkeypatch, dev, "drs_sep_project", project, lambda res: GC._within(res["out"], c["project"], "project"),
                   setup=hip_ops._SEP_WS.clear, case=str(shape))

    def project_eps(put):
        p = _guarded_projector(projector, put)
        x, t, ah = (put(c[k].to(dev)) for k in ("x", "t", "ah"))
        yt = hip_ops.sep_apply(put(c["y"].to(dev)), p.Pt_y, p.Pt_x)
        eps = hip_ops.lr_consistent_eps_(put(c["eps"].to(dev)), x, t, ah, yt, p, 1.0)
        return {"eps": eps, "x untouched": x, "strength 0": hip_ops.lr_consistent_eps_(put(c["eps"].to(dev)), x, t, ah, yt, p, 0.0)}
    G.guarded_runs(monkeypatch, dev, "drs_sep_project_eps", project_eps,
                   lambda res: GC._within(res["eps"], c["project_eps"], "project_eps"), setup=hip_ops._SEP_WS.clear, case=str(shape))
