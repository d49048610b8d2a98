"""The entry points of csrc/radiometry.hip between guard bands at the three pointer phases of tests/guard.py, run through
`test_gpu_guard.guarded_runs` - so that they count for that module's `test_every_entry_point_that_launches_is_guarded`, which
walks `_lib.SIGNATURES` and runs after this file (files run in name order; on its own that test does not know these entries).

Every mode must give the bits of the normal call: a pointer off its vector boundary makes a lane move its elements one by one
instead of at once, the same values through the same operations, and the histogram counts integers.  `shifted` puts the uint16
cache and the fp32 tensors at +4 bytes and the 64-bit counts at +8; the 2-byte phase of a uint16 cache - which the guards'
phases do not reach - is the odd-element view of tests/test_gpu_radiometry.py, repeated here inside a guarded copy."""
import numpy as np
import pytest
import torch

import radiometry_oracle as RO
import test_gpu_augment as GA
import test_gpu_guard as G
import test_gpu_radiometry as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _odd(put, cache, dev):
    """`cache` as a view that starts on the second element of a guarded buffer: the 2-byte pointer phase."""
    host = torch.from_numpy(np.concatenate([[0], cache.numpy().reshape(-1)]).astype(np.uint16))  # (assembled on the host)
    return put(host.to(dev))[1:].view(cache.shape)


@pytest.mark.parametrize("shape", [GA.SHAPES[0], GA.SHAPES[2], GA.SHAPES[4]], ids=str)
def test_crop_between_guards(monkeypatch, dev, shape):
    from diffusionremotesensing_amd import radiometry as R
    c, H, W, S = shape
    items, table = torch.from_numpy(GA._items(H, W, S)), R.check_table(TR._table(c))
    cache = TR._u16_cache((c, H, W), 90 + H, nodata=TR.K)
    want_hr, want_marked = RO.crop_mark(cache.numpy(), items.numpy(), S, table, TR.K)

    def oracle(res):
        TR._same_bits(res["hr"], want_hr, "hr")
        TR._same_marked(res["hr_marked"], want_marked, "hr_marked")

    def fn(put):
        it, td = put(items.to(dev)), put(torch.from_numpy(table).to(dev))
        hr, marked = R.crop_d4_u16_f32(put(cache.to(dev)), it, S, td, nodata=TR.K)
        odd_hr, odd_marked = R.crop_d4_u16_f32(_odd(put, cache, dev), it, S, td, nodata=TR.K)
        return {"hr": hr, "hr_marked": marked, "hr at an odd element": odd_hr, "hr_marked at an odd element": odd_marked,
                "hr alone": R.crop_d4_u16_f32(put(cache.to(dev)), it, S, td)[0]}
    G.guarded_runs(monkeypatch, dev, "drs_crop_d4_u16_f32", fn, oracle, case=str(shape))


@pytest.mark.parametrize("name", ["(2, 3, 5, 7)", "a constant plane"])
def test_hist_between_guards(monkeypatch, dev, name):
    from diffusionremotesensing_amd import radiometry as R
    cache = torch.from_numpy(TR._hist_cache(name))
    want = RO.histogram(cache.numpy())
    value = int(cache.reshape(-1)[0])
    want_nd = RO.histogram(cache.numpy(), value)

    def oracle(res):
        TR._same_bits(res["counts"], want, "counts")
        TR._same_bits(res["counts with nodata"], want_nd, "counts with nodata")

    def fn(put):
        return {"counts": R.hist_u16(put(cache.to(dev))), "counts at an odd element": R.hist_u16(_odd(put, cache, dev)),
                "counts with nodata": R.hist_u16(put(cache.to(dev)), nodata=value)}
    G.guarded_runs(monkeypatch, dev, "drs_hist_u16", fn, oracle, case=name)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 16, 8, 8)], ids=str)
def test_quantize_between_guards(monkeypatch, dev, shape):
    from diffusionremotesensing_amd import radiometry as R
    table = R.check_table(TR._table(shape[1]))
    rng = np.random.default_rng(sum(shape))
    x = (rng.random(shape) * 1.4 - 0.2).astype(np.float32)
    x.reshape(-1)[::11] = np.nan
    want = RO.quantize(x, table, fill=7, band_axis=1)

    def fn(put):
        return {"dn": R.quantize_u16(put(torch.from_numpy(x).to(dev)), put(torch.from_numpy(table).to(dev)), fill=7)}
    G.guarded_runs(monkeypatch, dev, "drs_quantize_u16", fn, lambda res: TR._same_bits(res["dn"], want, "dn"), case=str(shape))
