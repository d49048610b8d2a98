"""Stream ordering of the three entries of csrc/radiometry.hip: one late-input case each with tests/late.py, bit-equal to the
default-stream run - `row.crop_d4_u16`, `row.hist_u16` (whose memset of the counts must be on the caller's stream too) and
`row.quantize_u16`.

Registration.  tests/test_stream_order_host.py requires every entry of include/drs_hip.h with a `drs_stream_t` to be in
`test_gpu_stream_order.COVERAGE`, and every case named there to be a row of that module.  This module therefore registers, AT
IMPORT, its three entries in that module's COVERAGE, its row names in ROW_NAMES and its row builder in _BUILDERS - the same
cross-file arrangement the entry-guard files use with test_gpu_guard.  pytest imports every test file of the directory while
it collects (also under -m "not gpu"), so `python -m pytest tests -m "not gpu"` sees the rows and passes; that run of the whole
directory is the check.  tests/test_stream_order_host.py collected ALONE does not import this file, does not see the rows and
reports the three entries as uncovered.  The rows run here, not through `test_plan_less_entry`: that test's parameters were
fixed when its module was collected, before this one was imported (files are collected in name order).

The uint16 tensors travel through tests/late.py as int16 views of the same bits: its range check of integer inputs takes a
minimum, which torch does not have for uint16."""
import numpy as np
import pytest
import torch

import late
import test_gpu_stream_order as S

pytestmark = pytest.mark.gpu

ENTRIES = {"drs_crop_d4_u16_f32": "row.crop_d4_u16", "drs_hist_u16": "row.hist_u16", "drs_quantize_u16": "row.quantize_u16"}


def _rows_radiometry(dev):
    from diffusionremotesensing_amd import radiometry as R
    L, K = 5, 777

    def u16(seed):
        rng = np.random.default_rng(seed)
        cache = rng.integers(0, 65536, (L, 3, 9, 9)).astype(np.uint16)
        cache[:, :, 2:4, 3:6] = K  # no-data pixels
        return torch.from_numpy(cache.view(np.int16)).to(dev)
    cache, cache_stale = u16(1), u16(2)
    table = torch.tensor([[0.0, 65535.0], [123.0, 4567.0], [0.0, 10000.0]], device=dev)
    # (src, y0, x0, code): windows of 7 x 7 inside 9 x 9, as the rows of the 8-bit crops
    items = torch.tensor([[0, 0, 0, 0], [4, 2, 2, 7], [2, 1, 0, 3], [3, 0, 2, 5], [1, 2, 1, 6]], dtype=torch.int32, device=dev)
    items_stale = torch.tensor([[4, 2, 2, 1], [0, 0, 0, 2], [1, 0, 1, 4], [2, 2, 0, 0], [3, 1, 2, 3]], dtype=torch.int32, device=dev)
    whole = (-32768, 32767)
    rows = {}
    rows["crop_d4_u16"] = S._row(lambda b: R.crop_d4_u16_f32(b["cache"].view(torch.uint16), b["items"], 7, b["range"], nodata=K),
                                 {"cache": cache, "items": items, "range": table}, {"cache": cache_stale, "items": items_stale},
                                 {"cache": whole, "items": (0, 7)})
    rows["hist_u16"] = S._row(lambda b: R.hist_u16(b["cache"].view(torch.uint16), nodata=K), {"cache": cache}, {"cache": cache_stale},
                              {"cache": whole})
    x = S._rand(dev, "radiometry.x", (2, 3, 9, 13), -0.1, 1.1)
    rows["quantize_u16"] = S._row(lambda b: R.quantize_u16(b["x"], b["range"], fill=9).view(torch.int16), {"x": x, "range": table})
    return rows


# registration at import (see the module docstring)
for _entry, _case in ENTRIES.items():
    assert S.COVERAGE.setdefault(_entry, _case) == _case
for _case in ENTRIES.values():
    if _case[4:] not in S.ROW_NAMES:
        S.ROW_NAMES.append(_case[4:])
S.ROW_NAMES.sort()
if _rows_radiometry.__name__ not in {b.__name__ for b in S._BUILDERS}:
    S._BUILDERS = tuple(S._BUILDERS) + (_rows_radiometry,)


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
def test_radiometry_entry(dev, side, name):
    """One row per entry, every tensor input late, non-blocking: the entries do not synchronise the host."""
    case = f"row.{name}"
    with S._reaching(case):
        row = S._rows(dev)[name]
        _, _, group = late.check(row["fn"], row["inputs"], row["stale"], stream=side, ranges=row["ranges"], blocking=row["blocking"],
                                 must_sync=row["must_sync"], within=row["within"], reset=row["reset"], case=case)
        S._report(case)
        assert group == "bit-equal"
