"""Host side of the stream-order tests (no device): every entry of include/drs_hip.h that takes a `drs_stream_t` has a case in
tests/test_gpu_stream_order.py, and tests/late.py refuses inputs that could not prove anything or could fault."""
import os
import re

import pytest
import torch

import late
import test_gpu_stream_order as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entries_with_a_stream():
    header = open(os.path.join(ROOT, "include", "drs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"//[^\n]*", "", header)
    return {m.group(1) for m in re.finditer(r"\b(drs_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header, flags=re.S)
            if "drs_stream_t" in m.group(2)}


def test_every_entry_with_a_stream_has_a_stream_order_case():
    entries = _entries_with_a_stream()
    assert len(entries) >= 60 and "drs_unet_forward" in entries and "drs_sampler_step" in entries
    missing = sorted(entries - set(S.COVERAGE))
    assert not missing, f"entries of drs_hip.h that take a stream and have no stream-order case: {missing}"
    gone = sorted(set(S.COVERAGE) - entries)
    assert not gone, f"the coverage table names entries the header does not declare with a stream: {gone}"


def test_every_case_of_the_coverage_table_exists():
    """A case name is a test of the file: its rows, its chains and the named UNet / training tests."""
    source = open(os.path.join(ROOT, "tests", "test_gpu_stream_order.py")).read()
    named = set(re.findall(r'case = "([a-z0-9_.]+)"', source)) | set(re.findall(r'_reaching\("([a-z0-9_.]+)"\)', source))
    cases = named | {f"row.{n}" for n in S.ROW_NAMES} | {f"chain.{n}" for n in S.CHAINS}
    unknown = sorted((set(S.COVERAGE.values()) | S.UNMAPPED_CASES) - cases)
    assert not unknown, unknown
    assert not set(S.COVERAGE.values()) & S.UNMAPPED_CASES


def test_every_stream_entry_is_bound():
    from diffusionremotesensing_amd import _lib
    assert set(S.COVERAGE) <= set(_lib.SIGNATURES)


def _pair():
    inputs = {"x": torch.zeros(3, 4), "t": torch.tensor([3, 7, 11])}
    stale = {"x": torch.full((3, 4), float("nan")), "t": torch.tensor([5, 1, 20])}
    return inputs, stale


def test_legal_arguments_pass_on_the_host_form():
    inputs, stale = _pair()
    late.check_args(inputs, stale, {"t": (0, 49)}, require_device=False)
    assert late.stale_of(inputs, t=stale["t"])["x"].isnan().all()


def test_host_tensors_are_refused():
    inputs, stale = _pair()
    with pytest.raises(ValueError, match="device tensors"):
        late.check_args(inputs, stale, {"t": (0, 49)})


def test_name_mismatch_is_refused():
    inputs, stale = _pair()
    stale["y"] = stale.pop("x")
    with pytest.raises(ValueError, match="name different tensors"):
        late.check_args(inputs, stale, {"t": (0, 49)}, require_device=False)


@pytest.mark.parametrize("ranges, message", [(None, "needs ranges"), ({"t": (0, 11)}, "stale values 1 .. 20 leave"),
                                             ({"t": (4, 49)}, "input values 3 .. 11 leave"), ({"t": (0, 49), "x": (0, 1)}, "integer inputs")])
def test_integer_inputs_need_a_range_that_both_keep(ranges, message):
    inputs, stale = _pair()
    with pytest.raises(ValueError, match=message):
        late.check_args(inputs, stale, ranges, require_device=False)


def test_stale_values_must_differ_and_match_in_shape_and_type():
    inputs, stale = _pair()
    with pytest.raises(ValueError, match="equal the true ones"):
        late.check_args(inputs, dict(stale, t=inputs["t"].clone()), {"t": (0, 49)}, require_device=False)
    with pytest.raises(ValueError, match="stale is"):
        late.check_args(inputs, dict(stale, x=torch.zeros(3, 5)), {"t": (0, 49)}, require_device=False)
    with pytest.raises(ValueError, match="stale is"):
        late.check_args(inputs, dict(stale, t=stale["t"].int()), {"t": (0, 49)}, require_device=False)
    with pytest.raises(ValueError, match="give the stale values"):
        late.stale_of(inputs)


def test_the_spin_is_bounded():
    assert late.delay_ms_for(0.5) == late.MIN_DELAY_MS
    assert late.delay_ms_for(7.0) == 70.0
    with pytest.raises(AssertionError, match="chain.x.*split the case"):
        late.delay_ms_for(25.1, "chain.x")


def test_same_bits_compares_trees_by_their_bytes():
    a = {"y": [torch.tensor([1.0, float("nan")]), None, 3], "z": (torch.tensor([0.0]),)}
    b = {"y": [torch.tensor([1.0, float("nan")]), None, 3], "z": (torch.tensor([0.0]),)}
    assert late.same_bits(a, b)
    b["z"] = (torch.tensor([-0.0]),)
    assert not late.same_bits(a, b) and "out['z'][0]" in late._first_difference(a, b)
    assert issubclass(late.Inconclusive, AssertionError)
    with pytest.raises(AssertionError, match="names no tolerance"):
        late.compare(a, a, b, None, "case")
