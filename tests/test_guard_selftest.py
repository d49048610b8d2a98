"""tests/guard.py catches what it is there to catch (host only, CPU tensors).  Every planted change is an ordinary torch
index assignment on the parent buffer of a `Guarded`, inside its allocation."""
import struct

import pytest
import torch

import guard

CPU = torch.device("cpu")


def test_pattern_words_are_distinct_signalling_nans():
    w = guard.pattern_words(3 * 65536 + 5)
    assert w.dtype == torch.int32
    for i in (0, 1, 65535, 65536, 65537, 3 * 65536 + 4):
        assert int(w[i]) == 0x7FA00000 | (i & 0xFFFF)
    bits = w[:65536].to(torch.int64)
    assert bool(((bits >> 23) & 0xFF == 0xFF).all())  # exponent all ones
    assert bool(((bits >> 22) & 1 == 0).all())  # quiet bit clear
    assert bool((bits & 0x3FFFFF != 0).all())  # mantissa non-zero: NaN, not infinity
    assert torch.unique(w[:65536]).numel() == 65536
    assert bool((w[1:] != w[:-1]).all())  # no run of equal words matches it
    assert torch.isnan(w.view(torch.float32)).all()
    assert struct.unpack("<f", struct.pack("<I", 0x7FA00000 | 7))[0] != struct.unpack("<f", struct.pack("<I", 0x7FA00000 | 7))[0]


def test_float_read_modify_write_changes_a_guard_word():
    g = guard.Guarded((4,), torch.float32, CPU)
    assert g.damage() == []
    word = g.parent[g.end:g.end + 4].view(torch.float32)
    before = int(word.view(torch.int32)[0])
    word.add_(0.0)  # what an accumulate or an atomic add does to the word: the signalling NaN comes back quiet
    after = int(word.view(torch.int32)[0])
    assert after != before and after & 0x00400000
    assert g.damage() == [("after", 2, 2)]  # little endian: the quiet bit is in byte 2 of the word


@pytest.mark.parametrize("shift", [0, 4, 8])
@pytest.mark.parametrize("shape,dtype", [((3, 5), torch.float32), ((7,), torch.uint8), ((2, 3), torch.int64), ((0, 4), torch.float32)])
def test_guarded_layout(shape, dtype, shift):
    if shift % torch.empty((), dtype=dtype).element_size():
        with pytest.raises(ValueError):
            guard.Guarded(shape, dtype, CPU, shift)
        return
    g = guard.Guarded(shape, dtype, CPU, shift, fill="zero")
    v = g.view
    assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous()
    assert not v.numel() or bool((v == 0).all())
    if v.numel():
        assert v.data_ptr() % 256 == shift
        assert v.data_ptr() == g.parent.data_ptr() + g.start
        assert g.start >= guard.GUARD_BYTES >= 64 * 1024
        assert g.end + guard.GUARD_BYTES <= g.parent.numel()
    g.assert_intact()
    p = guard.Guarded(shape, dtype, CPU, shift)
    if dtype == torch.float32 and p.view.numel():
        assert torch.isnan(p.view).all()  # stands for torch.empty: unwritten output is NaN
    p.assert_intact()


POSITIONS = {  # name -> (parent index, side, offset in the report) of a Guarded g
    "one byte before": lambda g: (g.start - 1, "before", -1),
    "one byte after": lambda g: (g.end, "after", 0),
    "far end of the front guard": lambda g: (g.start - g.guard_bytes, "before", -g.guard_bytes),
    "far end of the back guard": lambda g: (g.end + g.guard_bytes - 1, "after", g.guard_bytes - 1),
}


@pytest.mark.parametrize("where", list(POSITIONS))
@pytest.mark.parametrize("shape,dtype,shift", [((5, 3), torch.float32, 4), ((13,), torch.uint8, 8), ((13,), torch.uint8, 0)])
def test_planted_byte_is_caught(where, shape, dtype, shift):
    g = guard.Guarded(shape, dtype, CPU, shift, what="the planted one")
    index, side, offset = POSITIONS[where](g)
    assert 0 <= index < g.parent.numel()
    g.parent[index] ^= 0x10
    assert g.damage() == [(side, offset, offset)]
    with pytest.raises(guard.GuardError) as e:
        g.assert_intact()
    msg = str(e.value)
    assert "the planted one" in msg and f"{offset:+d} .. {offset:+d}" in msg
    assert ("its start" if side == "before" else "its end") in msg
    g.parent[index] ^= 0x10
    g.assert_intact()


def test_damage_reports_first_and_last_byte():
    g = guard.Guarded((8,), torch.float32, CPU)
    g.parent[g.end + 4:g.end + 12] = 0
    g.parent[g.start - 16:g.start - 8] = 0
    assert g.damage() == [("before", -16, -9), ("after", 4, 11)]
    g.view.fill_(1.0)  # payload writes are what the buffer is for
    assert g.damage() == [("before", -16, -9), ("after", 4, 11)]


@pytest.mark.parametrize("mode", guard.MODES)
def test_factories(monkeypatch, mode):
    orig = {n: getattr(torch, n) for n in guard._FACTORIES}
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()  # not contiguous
    with guard.guarded_allocations(monkeypatch, CPU, mode) as block:
        made = {
            "empty": torch.empty((2, 3), dtype=torch.float32, device=CPU),
            "empty varargs": torch.empty(2, 3, dtype=torch.int32, device="cpu"),
            "bytes": torch.empty(100, dtype=torch.uint8, device=CPU),
            "zeros": torch.zeros(5, dtype=torch.float64, device=CPU),
            "zeros int": torch.zeros((1,), dtype=torch.int32, device=CPU),
            "ones": torch.ones((2, 2), dtype=torch.float32, device=CPU),
            "full": torch.full((3,), 2.5, dtype=torch.float32, device=CPU),
            "empty_like": torch.empty_like(src),
            "zeros_like": torch.zeros_like(src),
        }
        elsewhere = torch.empty(3)  # no device given: not the block's business
        assert len(block.allocations) == len(made)
        assert all("test_guard_selftest.py" in what for what, _ in block.allocations)
        shifts = [g.shift for _, g in block.allocations]
    for n in guard._FACTORIES:
        assert getattr(torch, n) is orig[n]
    assert elsewhere.shape == (3,)
    want = {"empty": ((2, 3), torch.float32), "empty varargs": ((2, 3), torch.int32), "bytes": ((100,), torch.uint8),
            "zeros": ((5,), torch.float64), "zeros int": ((1,), torch.int32), "ones": ((2, 2), torch.float32),
            "full": ((3,), torch.float32), "empty_like": ((4, 3), torch.float32), "zeros_like": ((4, 3), torch.float32)}
    for name, t in made.items():
        assert (tuple(t.shape), t.dtype) == want[name], name
        assert t.is_contiguous(), name
    for name in ("zeros", "zeros int", "zeros_like"):
        assert bool((made[name] == 0).all())
    assert bool((made["ones"] == 1).all()) and bool((made["full"] == 2.5).all())
    assert torch.isnan(made["empty"]).all()
    if mode == "aligned":
        assert shifts == [0] * 9
    elif mode == "shifted":
        assert shifts == [4, 4, 8, 8, 4, 4, 4, 4, 4]
    else:
        assert shifts == [0, 4, 0, 8, 0, 4, 0, 4, 0]
    for t, s in zip(made.values(), shifts):
        assert t.data_ptr() % 256 == s


def test_block_reports_the_damaged_allocation(monkeypatch):
    with pytest.raises(guard.GuardError) as e:
        with guard.guarded_allocations(monkeypatch, CPU, "shifted") as block:
            a = torch.empty(6, dtype=torch.float32, device=CPU)
            b = block.copy(torch.arange(5, dtype=torch.float32), "the input b")
            assert b.tolist() == [0, 1, 2, 3, 4] and b.data_ptr() % 256 == 4
            g = block.allocations[1][1]
            g.parent[g.end + 3] = 0  # the byte a store one element past b's end would end on
            a.fill_(0)
    msg = str(e.value)
    assert "the input b" in msg and "+3 .. +3" in msg and "test_block_reports" not in msg  # a is intact and not named
    assert torch.empty is guard._ORIG["empty"]


def test_untouched_block_passes_and_factories_return_after_an_exception(monkeypatch):
    with guard.guarded_allocations(monkeypatch, CPU, "mixed"):
        torch.zeros(4, dtype=torch.float32, device=CPU).add_(1)
    with pytest.raises(KeyError):
        with guard.guarded_allocations(monkeypatch, CPU, "mixed"):
            assert torch.empty is not guard._ORIG["empty"]
            raise KeyError("body")
    for n in guard._FACTORIES:
        assert getattr(torch, n) is guard._ORIG[n]


def test_library_proxy_records_calls(monkeypatch):
    from diffusionremotesensing_amd import _lib

    class Fake:
        def drs_abi_version(self):
            return 7
        other = 1
    monkeypatch.setattr(_lib, "load", lambda: Fake())
    with guard.guarded_allocations(monkeypatch, CPU, "aligned") as block:
        lib = _lib.load()
        assert lib.drs_abi_version() == 7 and lib.other == 1
        with pytest.raises(AttributeError):
            lib.drs_missing
    assert block.calls == {"drs_abi_version"}
    assert isinstance(_lib.load(), Fake)


def test_bits_equal():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert guard.bits_equal(a, a.clone())
    assert not guard.bits_equal(a, torch.tensor([1.0, float("nan"), 0.0]))
    assert not guard.bits_equal(a, a.double()) and not guard.bits_equal(a, a[:2])
    assert guard.bits_equal(None, None) and not guard.bits_equal(a, None)
