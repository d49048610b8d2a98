"""Sentinel guards around every buffer a test hands to the library: the memory-safety check of a project that cannot run a
GPU address sanitizer.

`Guarded` is one buffer laid out  guard | payload | guard,  filled with a pattern of 32-bit words that are signalling NaNs and
differ from word to word (`pattern_words`), the payload at a chosen pointer phase.  A plain store of any value changes a
word, a run of equal values cannot match the pattern, and a float read-modify-write quiets the NaN and so changes its bits
(tests/test_guard_selftest.py checks that last point with an in-place add).  Guards are compared as integers.

`guarded_allocations` swaps torch's factory functions for ones that return the interior view of a `Guarded`, so that every
output, workspace and packed image a wrapper of the package allocates is guarded by one mechanism, and reaches the ctypes
library through a proxy that records which `drs_*` entry points ran.

What it cannot see: an overrun from one tensor into the next INSIDE a workspace (one allocation), and an over-read whose
value does not reach a result.
"""
import contextlib
import traceback

import torch

GUARD_BYTES = 64 * 1024  # each side, at least
ALIGN = 256
PATTERN_BASE = 0x7FA00000  # exponent all ones, quiet bit clear, mantissa non-zero: a signalling NaN whatever the low 16 bits
MODES = ("aligned", "shifted", "mixed")
TYPED_SHIFT, BYTE_SHIFT = 4, 8  # "shifted": fp32 / int tensors at +4 bytes, byte buffers at the strictest documented alignment

_FACTORIES = ("empty", "empty_like", "zeros", "zeros_like", "full", "ones")
_ORIG = {name: getattr(torch, name) for name in _FACTORIES}  # the real ones, whatever is patched in later
_PATTERN_CACHE = {}  # device -> int32 pattern of the largest parent seen so far (the pattern has a period of 64 Ki words)


def pattern_words(n_words, device="cpu"):
    """int32 tensor of n_words pattern words: 0x7FA00000 | (word index & 0xFFFF)."""
    device = torch.device(device)
    have = _PATTERN_CACHE.get(device)
    if have is None or have.numel() < n_words:
        idx = torch.arange(max(n_words, 1 << 16), dtype=torch.int32, device=device)
        have = _PATTERN_CACHE[device] = torch.bitwise_or(torch.bitwise_and(idx, 0xFFFF), PATTERN_BASE)
    return have[:n_words]


def _itemsize(dtype):
    return _ORIG["empty"]((), dtype=dtype).element_size()


class GuardError(AssertionError):
    pass


class Guarded:
    """One buffer  guard | payload | guard.  `view` is the payload as a contiguous tensor of `shape` / `dtype` whose first
    byte sits at a 256-aligned address plus `shift`; `parent` (uint8) is the whole allocation.  fill="pattern" leaves the
    payload holding the pattern (it stands for torch.empty: what the kernel does not write stays NaN), fill="zero" clears it."""

    def __init__(self, shape, dtype, device, shift=0, fill="pattern", what="", guard_bytes=GUARD_BYTES):
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        item = _itemsize(dtype)
        if shift % item and numel:
            raise ValueError(f"shift {shift} is no multiple of {dtype}'s {item} bytes")
        self.nbytes = numel * item
        self.shift, self.what, self.guard_bytes = int(shift), what, int(guard_bytes)
        total = 2 * self.guard_bytes + self.nbytes + self.shift + 2 * ALIGN
        total = (total + 3) // 4 * 4
        words = _ORIG["empty"](total // 4, dtype=torch.int32, device=device)
        words.copy_(pattern_words(total // 4, words.device))
        self.parent = words.view(torch.uint8)
        base = self.parent.data_ptr()
        if base % 4:
            raise RuntimeError("the allocator returned a pointer that is not 4-byte aligned")
        start = (base + self.guard_bytes + ALIGN - 1) // ALIGN * ALIGN + self.shift - base
        self.start, self.end = start, start + self.nbytes
        payload = self.parent[self.start:self.end]
        if fill == "zero":
            payload.zero_()
        elif fill != "pattern":
            raise ValueError(fill)
        self.view = payload.view(dtype).view(shape) if numel else _ORIG["empty"](shape, dtype=dtype, device=device)
        assert not numel or (self.view.data_ptr() - self.shift) % ALIGN == 0
        assert self.view.is_contiguous()

    def damage(self):
        """[(side, first, last)] of the damaged guards: byte offsets relative to the payload's start ("before", negative) or
        to its end ("after", from 0)."""
        want = pattern_words(self.parent.numel() // 4, self.parent.device).view(torch.uint8)
        out = []
        for side, lo, hi, origin in (("before", self.start - self.guard_bytes, self.start, self.start),
                                     ("after", self.end, self.end + self.guard_bytes, self.end)):
            bad = torch.nonzero(self.parent[lo:hi] != want[lo:hi]).flatten()  # uint8 against uint8: integers
            if bad.numel():
                out.append((side, int(bad[0]) + lo - origin, int(bad[-1]) + lo - origin))
        return out

    def assert_pattern(self, lo, hi, what):
        """The payload bytes [lo, hi) still hold the pattern: a gap between two tensors that share this buffer."""
        want = pattern_words(self.parent.numel() // 4, self.parent.device).view(torch.uint8)
        a, b = self.start + lo, self.start + hi
        bad = torch.nonzero(self.parent[a:b] != want[a:b]).flatten()
        if bad.numel():
            raise GuardError(f"gap damaged {what}: payload bytes {int(bad[0]) + lo} .. {int(bad[-1]) + lo} of the gap {lo} .. {hi}")

    def assert_intact(self, what=None):
        dmg = self.damage()
        if dmg:
            text = "; ".join(f"{side} the payload: bytes {first:+d} .. {last:+d} relative to its {'start' if side == 'before' else 'end'}"
                             for side, first, last in dmg)
            raise GuardError(f"guard damaged around {what or self.what} ({self.nbytes} payload bytes at 256k+{self.shift}): {text}")


def bits_equal(a, b):
    """Same shape, dtype and bytes (NaNs compare by their bits)."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8).cpu(),
                       b.detach().contiguous().reshape(-1).view(torch.uint8).cpu())


def _call_site():
    """file:line (function) of the innermost frame outside this module and torch."""
    for fr in reversed(traceback.extract_stack()[:-2]):
        if fr.filename != __file__ and "/torch/" not in fr.filename and "contextlib" not in fr.filename:
            return f"{fr.filename.rsplit('/', 1)[-1]}:{fr.lineno} ({fr.name})"
    return "?"


class _RecordingLib:
    """The ctypes library behind a proxy that notes the name of every drs_* function fetched for a call."""

    def __init__(self, real, calls):
        self.__dict__["_real"], self.__dict__["_calls"] = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("drs_"):
            self._calls.add(name)
        return fn


class GuardedBlock:
    """State of one `guarded_allocations` block: `allocations` [(call site, Guarded)], `calls` the drs_* names used."""

    def __init__(self, dev, mode):
        if mode not in MODES:
            raise ValueError(f"mode {mode!r} must be one of {MODES}")
        self.dev, self.mode = torch.device(dev), mode
        self.allocations, self.calls, self._count = [], set(), 0

    def _shift(self, dtype):
        """Typed tensors move by 4 bytes (64-bit ones by 8: a pointer to int64 / double stays one), byte buffers by 8."""
        typed = max(TYPED_SHIFT, _itemsize(dtype))
        if self.mode == "aligned":
            return 0
        if self.mode == "shifted":
            return BYTE_SHIFT if dtype in (torch.uint8, torch.int8) else typed
        self._count += 1  # mixed: 0, 4, 0, 4, ... (a byte buffer: 0 or 8, no entry point takes a workspace at less)
        return 0 if self._count % 2 else (BYTE_SHIFT if dtype in (torch.uint8, torch.int8) else typed)

    def alloc(self, shape, dtype, fill, what=None, shift=None):
        g = Guarded(shape, dtype, self.dev, self._shift(dtype) if shift is None else shift, fill, what or _call_site())
        self.allocations.append((g.what, g))
        return g.view

    def copy(self, t, what=None, shift=None):
        """`t` (a tensor on the block's device, or None) in a guarded buffer of its own, at this block's pointer phase (or
        at 256 k + `shift` bytes)."""
        if t is None:
            return None
        out = self.alloc(t.shape, t.dtype, "pattern", what or f"copy at {_call_site()}", shift)
        out.copy_(t)
        return out.requires_grad_(t.requires_grad) if t.is_floating_point() else out

    def assert_intact(self):
        errors = []
        for what, g in self.allocations:
            try:
                g.assert_intact(what)
            except GuardError as e:
                errors.append(str(e))
        if errors:
            raise GuardError("\n".join(errors))

    # -- the factories ------------------------------------------------------------------------------------------------
    def _mine(self, device):
        if device is None:
            return False
        device = torch.device(device)
        if device.type != self.dev.type:
            return False
        if device.type == "cpu":
            return True
        index = device.index if device.index is not None else torch.cuda.current_device()
        return index == (self.dev.index if self.dev.index is not None else torch.cuda.current_device())

    @staticmethod
    def _size(args, kw):
        if "size" in kw:
            return tuple(kw.pop("size")), args
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            return tuple(args[0]), ()
        return tuple(args), ()

    def _plain(self, kw):  # only the keywords the package uses: anything else goes to the real factory
        return not (set(kw) - {"dtype", "device", "requires_grad"}) and not kw.get("requires_grad", False)

    def _sized(self, name, fill):
        orig = _ORIG[name]

        def factory(*args, **kw):
            if not self._mine(kw.get("device")) or not self._plain({k: v for k, v in kw.items() if k != "size"}):
                return orig(*args, **kw)
            kw = dict(kw)
            size, _ = self._size(args, kw)
            if not all(isinstance(s, int) or hasattr(s, "__index__") for s in size):
                return orig(*args, **kw)
            out = self.alloc(size, kw.get("dtype") or torch.get_default_dtype(), "zero" if fill == 0 else "pattern")
            return out.fill_(fill) if fill not in (None, 0) else out
        return factory

    def _full(self):
        orig = _ORIG["full"]

        def full(size, fill_value, **kw):
            if not self._mine(kw.get("device")) or not self._plain(kw):
                return orig(size, fill_value, **kw)
            dtype = kw.get("dtype") or orig((), fill_value).dtype
            return self.alloc(tuple(size), dtype, "pattern").fill_(fill_value)
        return full

    def _like(self, name, fill):
        orig = _ORIG[name]

        def like(t, **kw):
            device = kw.get("device", t.device)
            fmt = kw.get("memory_format", torch.contiguous_format)
            dense = fmt == torch.contiguous_format or (fmt == torch.preserve_format and t.is_contiguous())
            if not self._mine(device) or (set(kw) - {"dtype", "device", "memory_format"}) or t.layout != torch.strided or not dense:
                return orig(t, **kw)
            return self.alloc(t.shape, kw.get("dtype") or t.dtype, "zero" if fill == 0 else "pattern")
        return like

    def factories(self):
        return {"empty": self._sized("empty", None), "zeros": self._sized("zeros", 0), "ones": self._sized("ones", 1),
                "full": self._full(), "empty_like": self._like("empty_like", None), "zeros_like": self._like("zeros_like", 0)}


@contextlib.contextmanager
def guarded_allocations(monkeypatch, dev, mode):
    """Inside the block torch.empty / empty_like / zeros / zeros_like / full / ones return guarded tensors for `dev`, and
    `_lib.load()` returns a recording proxy.  On exit the originals are back (also after an exception) and, when the body
    did not raise, every guard is checked.  Yields the `GuardedBlock`."""
    from diffusionremotesensing_amd import _lib
    block = GuardedBlock(dev, mode)
    real_load = _lib.load
    with monkeypatch.context() as mp:
        for name, fn in block.factories().items():
            mp.setattr(torch, name, fn)
        mp.setattr(_lib, "load", lambda: _RecordingLib(real_load(), block.calls))
        yield block
    block.assert_intact()


def guarded_copy(t, block):
    """`t` in a guarded buffer of `block` (checked with the block's other guards on exit); None stays None."""
    return block.copy(t)
