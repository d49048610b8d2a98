"""Late inputs: the stream-order check of a library whose every entry takes a stream and runs part of its work on streams of
its own.

`run(fn, inputs, stale, stream=...)` owns the buffers `fn` sees.  They hold `stale` - legal but different values - while a spin
kernel (`torch.cuda._sleep`) occupies `stream`; the copies of the true values stand behind the spin on the same stream, and
`fn` is called while the device still spins.  Work that `fn` orders after what is already enqueued on the current stream sees
the true values.  Anything it runs out of order - a launch on stream 0, a side stream that does not wait for the caller's, a
memset on the wrong stream - finishes during the spin, on stale inputs, and the result differs from `baseline` by far more than
rounding.  The outputs are cloned on `stream` right behind the call and only then is the stream (never the device) waited for,
so work left on an un-joined side stream is not hidden by the harness either.

The run is valid only if the host returned from `fn` while the spin was still going: `ev_fed.query()` is read when `fn`
returns.  True means the run proved nothing (`Inconclusive`, an AssertionError: a failure, not a skip) - and the same check pins
that the entry does not synchronise the host.  The event is also read in front of the first library call
(`note_library_call`): there it must be pending for every case, since a host wait before the first launch leaves nothing to
order; a case that is expected to call the library and whose calls never pass the proxy fails as well.  Entries that read back
to the host by design run with blocking=True, where the comparison with the baseline carries the test; `must_sync=True` turns
the check round for an entry that promises to have waited for `stream` when it returns.

Stale values must be legal: a missed wait has to give wrong numbers, never a memory fault.  Integer inputs therefore need a
range, which both the true and the stale values are checked against (`check_args`, which runs on the host as well).

What it cannot see: hazards that depend on the relative speed of two streams INSIDE one call.
"""
import time

import torch

MIN_DELAY_MS = 20.0
MAX_DELAY_MS = 250.0
HOST_FACTOR = 10.0
WARM_CALLS = 3

RECORDS = []  # one dict per `run`: case, host_ms, delay_ms, fed (ev_fed.query() when fn returned)
_CYCLES_PER_MS = {}  # device index -> spin cycles per millisecond


class Inconclusive(AssertionError):
    """The device had left the spin before `fn` returned: the run ordered nothing (or `fn` synchronised the host)."""


def _is_integer(t):
    return not (t.is_floating_point() or t.is_complex())


def check_args(inputs, stale, ranges=None, require_device=True):
    """ValueError / TypeError unless `stale` names the tensors of `inputs`, one for one in shape, dtype and device, differs
    from them, and every integer tensor (timesteps, labels, masks, bytes, origins) has an inclusive range in `ranges` that its
    true and its stale values both keep."""
    ranges = ranges or {}
    if not isinstance(inputs, dict) or not isinstance(stale, dict):
        raise TypeError("inputs and stale are dicts of name -> tensor")
    if set(inputs) != set(stale):
        raise ValueError(f"inputs and stale name different tensors: {sorted(set(inputs) ^ set(stale))}")
    if set(ranges) - set(inputs):
        raise ValueError(f"ranges given for unknown inputs: {sorted(set(ranges) - set(inputs))}")
    for name, true in inputs.items():
        old = stale[name]
        if not isinstance(true, torch.Tensor) or not isinstance(old, torch.Tensor):
            raise TypeError(f"{name}: inputs and stale hold tensors")
        if true.shape != old.shape or true.dtype != old.dtype or true.device != old.device:
            raise ValueError(f"{name}: stale is {tuple(old.shape)} {old.dtype} on {old.device}, the input "
                             f"{tuple(true.shape)} {true.dtype} on {true.device}")
        if _is_integer(true):
            if name not in ranges:
                raise ValueError(f"{name}: an integer input needs ranges[{name!r}] = (lo, hi): a stale value must not be able to "
                                 "index outside a table or a tensor")
            lo, hi = ranges[name]
            for what, t in (("input", true), ("stale", old)):
                if t.numel() and (int(t.min()) < lo or int(t.max()) > hi):
                    raise ValueError(f"{name}: the {what} values {int(t.min())} .. {int(t.max())} leave the legal range {lo} .. {hi}")
        elif name in ranges:
            raise ValueError(f"{name}: ranges are for integer inputs")
        if true.numel() and torch.equal(true, old):  # (NaN != NaN: a NaN-filled stale tensor always differs)
            raise ValueError(f"{name}: the stale values equal the true ones")
    if require_device:
        for name, true in inputs.items():
            if not true.is_cuda:
                raise ValueError(f"{name} is on {true.device}: late inputs are device tensors (a host-to-device copy would block)")


def nan_like(t):
    return torch.full_like(t, float("nan"))


def stale_of(inputs, **given):
    """NaN for every float tensor of `inputs`; the integer ones must be `given`."""
    out = {}
    for name, t in inputs.items():
        if name in given:
            out[name] = given[name]
        elif t.is_floating_point():
            out[name] = nan_like(t)
        else:
            raise ValueError(f"{name}: give the stale values of an integer input")
    return out


def cycles_per_ms(device=None):
    """Spin cycles of torch.cuda._sleep per millisecond, measured once per device with two timing events."""
    index = torch.cuda.current_device() if device is None else torch.device(device).index or 0
    have = _CYCLES_PER_MS.get(index)
    if have is not None:
        return have
    with torch.cuda.device(index):
        torch.cuda._sleep(1000)
        n, ms = 1_000_000, 0.0
        for _ in range(4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= 5.0:
                break
            n = int(n * max(2.0, 10.0 / max(ms, 1e-3)))
        if ms < 1.0:
            raise AssertionError(f"torch.cuda._sleep({n}) took {ms:.3f} ms: cannot calibrate the spin")
        _CYCLES_PER_MS[index] = n / ms
    return _CYCLES_PER_MS[index]


def delay_ms_for(host_ms, case=""):
    delay = max(MIN_DELAY_MS, HOST_FACTOR * host_ms)
    if delay > MAX_DELAY_MS:
        raise AssertionError(f"{case}: one warm call takes {host_ms:.2f} ms on the host, the spin would be {delay:.0f} ms "
                             f"(limit {MAX_DELAY_MS:.0f} ms): split the case")
    return delay


def _map(out, f):
    if isinstance(out, torch.Tensor):
        return f(out)
    if isinstance(out, (tuple, list)):
        return type(out)(_map(o, f) for o in out)
    if isinstance(out, dict):
        return {k: _map(v, f) for k, v in out.items()}
    return out  # None and host scalars


def _clone(out):
    return _map(out, lambda t: t.detach().clone())


def _fresh(tensors):
    return {k: v.detach().clone() for k, v in tensors.items()}


def baseline(fn, inputs, reset=None):
    """`fn` on copies of the true values, on the default stream, the device idle before and after.  `reset()`, when given,
    runs before `fn` (a case with state of its own puts it back)."""
    torch.cuda.synchronize()
    if reset is not None:
        reset()
    out = _clone(fn(_fresh(inputs)))
    torch.cuda.synchronize()
    return out


def warm_values(inputs, stale):
    """A third set of legal values, for the warm-up: the finite floats of `inputs` moved (0.75 v + 0.125: data in [0, 1] stays
    there), its integers those of `stale`.  The late run then meets a library whose workspaces, tables and caches hold the
    results of OTHER data: a kernel that reads an intermediate too early cannot find this call's right answer there."""
    out = {}
    for name, t in inputs.items():
        out[name] = torch.where(torch.isfinite(t), t * 0.75 + 0.125, t) if t.is_floating_point() else stale[name].clone()
    return out


_ACTIVE = None  # the late run in progress: its arrival events, and whether they had completed at the first library call


def note_library_call():
    """Called by the tests' library proxy in front of every entry that takes a stream: the first one of a late run records
    whether the inputs had already arrived.  They must not have, blocking entry or not: a host wait in FRONT of the first
    launch means that nothing was ordered against the late inputs."""
    if _ACTIVE is not None and _ACTIVE["first"] is None:
        _ACTIVE["first"] = any(ev.query() for ev in _ACTIVE["events"])


class Job:
    """One `fn` with its true and stale inputs and the stream it is called on (`run_many`)."""

    def __init__(self, fn, inputs, stale, stream, ranges=None, reset=None):
        check_args(inputs, stale, ranges)
        if stream == torch.cuda.default_stream():
            raise ValueError("late inputs arrive on a stream other than the default one")
        self.fn, self.inputs, self.stale, self.stream, self.reset = fn, inputs, stale, stream, reset


def run_many(jobs, *, blocking=False, case="", must_sync=False, library=True):
    """[outputs of job.fn(buffers)] with every job's true values arriving behind a spin on its own stream; all spins are
    enqueued first, then the jobs are called in order, then all `ev_fed` are read: every job was enqueued before any spin ended.
    Each `fn` runs WARM_CALLS times on its stream with `warm_values` first: the warm-up, and two calls of which the faster one's
    host time sizes the spin."""
    global _ACTIVE
    per_ms = cycles_per_ms()
    staging = [_fresh(j.inputs) for j in jobs]  # device-resident: the late copies are device-to-device
    warm = [warm_values(j.inputs, j.stale) for j in jobs]
    torch.cuda.synchronize()
    host_ms = 0.0
    for j, values in zip(jobs, warm):
        with torch.cuda.stream(j.stream):
            times = []
            for _ in range(WARM_CALLS):
                if j.reset is not None:
                    j.reset()
                bufs = _fresh(values)
                t0 = time.perf_counter()
                out = j.fn(bufs)
                times.append((time.perf_counter() - t0) * 1e3)
                # the warm outputs are overwritten, behind the call on its stream, before their memory goes back to the
                # allocator: the late run's outputs land on these blocks and must not find an answer there (a `fn` that
                # returns live state has a `reset` that restores it), and no call pays for fresh device allocations
                with torch.no_grad():
                    _map((bufs, out), lambda t: t.detach().fill_(float("nan")) if t.is_floating_point() else t.detach().zero_())
                del bufs, out
            host_ms += min(times[1:])  # (the first call pays for plans, packing and allocations; a hiccup in one is not the entry's)
    torch.cuda.synchronize()
    delay = delay_ms_for(host_ms, case)
    buffers, events, got = [], [], []
    for j in jobs:
        if j.reset is not None:
            with torch.cuda.stream(j.stream):
                j.reset()
        buffers.append(_fresh(j.stale))
        events.append(torch.cuda.Event())
    torch.cuda.synchronize()
    for j, staged, bufs, ev in zip(jobs, staging, buffers, events):
        with torch.cuda.stream(j.stream):
            torch.cuda._sleep(int(delay * per_ms))
            for name, t in bufs.items():
                t.copy_(staged[name], non_blocking=True)
            ev.record(j.stream)
    outs = []
    _ACTIVE = probe = {"events": events, "first": None}
    try:
        for j, bufs in zip(jobs, buffers):
            with torch.cuda.stream(j.stream):
                outs.append(j.fn(bufs))
    finally:
        _ACTIVE = None
    fed = [ev.query() for ev in events]  # (before the clones: their fresh allocations cost host time that is not the entry's)
    for j, out in zip(jobs, outs):
        with torch.cuda.stream(j.stream):
            got.append(_clone(out))  # the clone is the first consumer, ordered by the stream alone
    for j in jobs:
        j.stream.synchronize()
    RECORDS.append({"case": case, "host_ms": host_ms, "delay_ms": delay, "fed": any(fed), "blocking": blocking})
    if library and probe["first"] is None:
        raise AssertionError(f"{case}: no library call passed the recording proxy during the late run, so nothing says whether "
                             "the inputs were still pending at the first one (library=False is for cases of plain torch)")
    if probe["first"]:
        raise Inconclusive(f"{case}: the true inputs had arrived before fn made its first library call: something in front of it "
                           "made the host wait for the stream (an upload from pageable memory, a read-back), and no launch of the "
                           "entry was ordered against the late inputs")
    if not blocking and any(fed):
        raise Inconclusive(f"{case}: the true inputs had arrived when fn returned (host time of a warm call {host_ms:.2f} ms, spin "
                           f"{delay:.0f} ms): the entry synchronised the host, or the run proved nothing")
    if must_sync and not all(fed):
        raise AssertionError(f"{case}: fn returned while the work enqueued on its stream was still pending, although the entry "
                             "promises to have waited for that stream")
    return got


def run(fn, inputs, stale, *, stream, blocking=False, ranges=None, case="", must_sync=False, reset=None, library=True):
    """The outputs of `fn(buffers)` (a tensor, or tuples / lists / dicts of tensors, None and host scalars) with the true values
    of `inputs` arriving behind a spin on `stream`; see the module docstring."""
    return run_many([Job(fn, inputs, stale, stream, ranges, reset)], blocking=blocking, case=case, must_sync=must_sync,
                    library=library)[0]


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b):
    """Trees of the same structure whose tensors have the same shape, dtype and bytes (NaN compares by its bits), and whose
    other leaves are equal."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
                and bool(torch.equal(_bits(a), _bits(b))))
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return a == b


def compare(got, base1, base2, within=None, case=""):
    """The comparison rule: two baselines with the same bits oblige the late result to their bits; otherwise (an op that adds
    with atomics) `within(got, base1, base2)` must hold - the bar of the op's own GPU test.  Returns the group, "bit-equal" or
    "tolerance"."""
    if same_bits(base1, base2):
        assert same_bits(got, base1), f"{case}: the late result differs from the default-stream result{_first_difference(got, base1)}"
        group = "bit-equal"
    else:
        assert within is not None, f"{case}: two default-stream runs differ and the case names no tolerance"
        within(got, base1, base2)
        group = "tolerance"
    if RECORDS and RECORDS[-1]["case"] == case:
        RECORDS[-1]["group"] = group
    return group


def _first_difference(a, b, path="out"):
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        if a.shape != b.shape or a.dtype != b.dtype:
            return f" ({path}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype})"
        if torch.equal(_bits(a), _bits(b)):
            return ""
        fa, fb = a.double().flatten(), b.double().flatten()
        bad = ~((fa == fb) | (torch.isnan(fa) & torch.isnan(fb)))
        i = int(torch.nonzero(bad)[0]) if bool(bad.any()) else 0
        return (f" ({path}: {int(bad.sum())} of {fa.numel()} elements differ, the first at {i}: {fa[i].item()!r} against "
                f"{fb[i].item()!r}; {int(torch.isnan(fa).sum())} NaN in the late result)")
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        for k, (x, y) in enumerate(zip(a, b)):
            d = _first_difference(x, y, f"{path}[{k}]")
            if d:
                return d
    if isinstance(a, dict) and isinstance(b, dict):
        for k in a:
            d = _first_difference(a[k], b.get(k), f"{path}[{k!r}]")
            if d:
                return d
    return "" if same_bits(a, b) else f" ({path}: {a!r} against {b!r})"


def check(fn, inputs, stale, *, stream, blocking=False, ranges=None, case="", within=None, must_sync=False, reset=None,
          library=True):
    """Two baselines, one late run, the comparison rule.  Returns (late outputs, baseline outputs, group)."""
    base1 = baseline(fn, inputs, reset)
    base2 = baseline(fn, inputs, reset)
    got = run(fn, inputs, stale, stream=stream, blocking=blocking, ranges=ranges, case=case, must_sync=must_sync, reset=reset,
              library=library)
    return got, base1, compare(got, base1, base2, within, case)
