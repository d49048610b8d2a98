"""Stream ordering of the four entries of the sensor-MTF degradation: one late-input case each with tests/late.py, bit-equal
to the default-stream run - `row.fir_decimate`, `row.sep_apply_bands`, `row.sep_project_bands`, `row.lr_consistent_eps_bands`.

Registration is that of tests/test_gpu_stream_order_radiometry.py (see its docstring): tests/test_stream_order_host.py requires
every entry of include/drs_hip.h with a `drs_stream_t` to be in `test_gpu_stream_order.COVERAGE`, so this module registers, AT
IMPORT, its entries there, its row names in ROW_NAMES and its row builder in _BUILDERS; the run of the whole directory is the
check, and the rows run here."""
import pytest
import torch

import late
import mtf_oracle as MO
import test_gpu_stream_order as S

pytestmark = pytest.mark.gpu

ENTRIES = {"drs_fir_decimate": "row.fir_decimate", "drs_sep_apply_bands": "row.sep_apply_bands",
           "drs_sep_project_bands": "row.sep_project_bands", "drs_sep_project_eps_bands": "row.lr_consistent_eps_bands"}
GAINS = (0.35, 0.2, 0.35)


def _rows_mtf(dev):
    from diffusionremotesensing_amd import hip_ops as H
    from diffusionremotesensing_amd.consistency import BandOperator
    taps, L, band_op = MO.band_taps(GAINS, 2)
    rows_t = torch.from_numpy(taps).float().to(dev)
    sigma = torch.tensor([0.0, 0.02, 0.05], device=dev)
    x = S._rand(dev, "mtf.x", (2, 3, 24, 24), 0.0, 1.0)
    y = S._rand(dev, "mtf.y", (2, 3, 12, 12), 0.0, 1.0)
    projector = BandOperator.mtf((24, 24), 2, GAINS).projector(0.01, dev)
    _, ah, _ = S._schedule(dev)
    rows = {}
    rows["fir_decimate"] = S._row(lambda b: H.fir_decimate(b["x"], b["ky"], b["kx"], L, 2, band_op=band_op, noise=b["z"], sigma=b["sigma"],
                                                           clamp=True),
                                  {"x": x, "ky": rows_t, "kx": rows_t.clone(), "z": S._rand(dev, "mtf.z", (2, 3, 12, 12)), "sigma": sigma})
    rows["sep_apply_bands"] = S._row(lambda b: H.sep_apply(b["x"], projector.D_y, projector.D_x, band_op=band_op), {"x": x})
    rows["sep_project_bands"] = S._row(lambda b: H.sep_project(b["x"], projector.prepare(b["y"]), projector, 0.8), {"x": x, "y": y})
    t, t_stale = S._levels(dev, "mtf", 2)
    rows["lr_consistent_eps_bands"] = S._row(
        lambda b: H.lr_consistent_eps_(b["eps"], b["x"], b["t"], ah, projector.prepare(b["y"]), projector, 0.8),
        {"eps": S._rand(dev, "mtf.eps", (2, 3, 24, 24)), "x": x, "y": y, "t": t}, {"t": t_stale}, {"t": (0, S.T - 1)})
    return rows


# registration at import (see the module docstring)
for _entry, _case in ENTRIES.items():
    assert S.COVERAGE.setdefault(_entry, _case) == _case
for _case in ENTRIES.values():
    if _case[4:] not in S.ROW_NAMES:
        S.ROW_NAMES.append(_case[4:])
S.ROW_NAMES.sort()
if _rows_mtf.__name__ not in {b.__name__ for b in S._BUILDERS}:
    S._BUILDERS = tuple(S._BUILDERS) + (_rows_mtf,)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    late.cycles_per_ms()
    return torch.device("cuda:0")


@pytest.fixture()
def side(dev):
    return torch.cuda.Stream(dev)


@pytest.mark.parametrize("name", [c[4:] for c in ENTRIES.values()])
def test_mtf_entry(dev, side, name):
    """One row per entry, every tensor input late, non-blocking: the entries do not synchronise the host."""
    case = f"row.{name}"
    with S._reaching(case):
        row = S._rows(dev)[name]
        _, _, group = late.check(row["fn"], row["inputs"], row["stale"], stream=side, ranges=row["ranges"], blocking=row["blocking"],
                                 must_sync=row["must_sync"], within=row["within"], reset=row["reset"], case=case)
        S._report(case)
        assert group == "bit-equal"
