"""Every buffer the library writes sits between sentinel guards (tests/guard.py), at three pointer phases.

Each case runs once the normal way and once per mode inside `guarded_allocations`: outputs, workspaces, packed images and
the tensors the test passes in are then interior views of guarded buffers - 256-aligned (`aligned`), 4 bytes (byte buffers: 8)
past a 256-byte boundary (`shifted`: the alignment reserves of the `*_bytes` contracts are nearly used up, every launcher
that picks a vector path from pointer alignment takes its element-by-element one), or alternating between the two (`mixed`:
the tensors of one call at different phases).  The guards must be intact and the results equal bit for bit to the normal call's.
The shapes are those an existing test already holds to a float64 oracle (imported from its table where it keeps one); where
that is not so, the normal call is compared with the op's oracle at that test's bar here, so the bitwise match inherits it.

EXCEPTIONS lists, per (function, mode), the two permitted departures: the wrapper refuses the pointer with its documented
error, or the scalar and vector paths sum in a different order and both results are held to the oracle instead.  The last
test asserts that every entry point that launches anything ran inside a guarded block.
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import guard
from guard import MODES, bits_equal, guarded_allocations

pytestmark = pytest.mark.gpu

ORDER = "order depends on path"
_ATOMICS = ("the weight, bias and BatchNorm-affine gradients are reduced with float atomicAdd (wgrad_mfma / wgrad_direct split-K, "
            "colsum, time_mlp_bwd): the order of the addends changes from launch to launch, two NORMAL steps already differ in "
            "their last bits (measured: 72 of 176 tensors of `tiny`, by at most 5e-9), so no path can be compared bit for bit; "
            "prediction, loss and running statistics are bit-equal")
# (function, mode) -> ("refused", the documented error) | (ORDER, why).  Nothing else may differ from the normal call.
_SCALAR = ("with H W % 4 == 0 the misaligned pointers select the element-by-element instance, whose threads cover other elements "
           "than the float4 instance's: the double partial sums are added in another order")
EXCEPTIONS = {
    **{("unet_train_step", m): (ORDER, _ATOMICS) for m in MODES},
    ("unet_backward_slots", "aligned"): (ORDER, _ATOMICS),
    # measured on the 64 x 64 image: PSNR 1.2e-7 dB, SAM 1.3e-6 degrees, ERGAS 5.9e-7 apart; SSIM (one path) bit-equal
    **{("metrics_pointwise+ssim", m): (ORDER, "the per-image sums of metrics_pointwise: " + _SCALAR) for m in ("shifted", "mixed")},
    # measured at (2, 3, 16, 20): the per-image sums 5.7e-14 apart; every map and the rank histogram bit-equal
    **{("ensemble_stats+scores", m): (ORDER, "the per-image sums of ensemble_scores: " + _SCALAR) for m in ("shifted", "mixed")},
    # measured at (5, 16, 8, 8): per-image losses and the bins' sums / rings 1.1e-16 apart; the gradient bit-equal
    **{("diffusion_loss", m): (ORDER, "the per-image losses, and the loss and the bins that are made of them: a row that starts off "
                                      "a 16-byte boundary is cut into head, float4 groups and tail, so the partial sums cover other "
                                      "elements (in `mixed` pred and target take the phases of the normal call's sums: bit-equal)")
       for m in ("shifted",)},
}

_RECORDED = set()  # drs_* names called inside guarded blocks, by every test of this module


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sds(seeded_sd, seeded_sd_sar, seeded_sd_gen):
    return {"superres": seeded_sd, "sar": seeded_sd_sar, "generation": seeded_sd_gen}


def _normal(t, **kw):
    return t


def _differing(ref, got):
    assert set(ref) == set(got), sorted(set(ref) ^ set(got))
    return [k for k in ref if not bits_equal(ref[k], got[k])]


def _describe(ref, got, names):
    out = []
    for k in names[:6]:
        a, b = ref[k], got[k]
        if a is None or b is None or a.shape != b.shape or not a.dtype.is_floating_point:
            out.append(f"{k}: {None if a is None else tuple(a.shape)} / {None if b is None else tuple(b.shape)}")
            continue
        d = (a.double() - b.double()).abs()
        bad = torch.nonzero(~((a == b) | (torch.isnan(a) & torch.isnan(b))).reshape(-1)).flatten()
        out.append(f"{k}: {bad.numel()} of {a.numel()} elements differ, flat index {int(bad[0]) if bad.numel() else '-'} .. "
                   f"{int(bad[-1]) if bad.numel() else '-'}, max |diff| {d[~torch.isnan(d)].max().item() if (~torch.isnan(d)).any() else 'nan'}")
    return "; ".join(out) + (f" (+{len(names) - 6} more)" if len(names) > 6 else "")


def guarded_runs(monkeypatch, dev, function, fn, oracle=None, modes=MODES, setup=None, case="", unordered=None, one_path=False):
    """`fn(put)` -> {result name: tensor | None}: builds its inputs, passes every device tensor it hands to the library through
    `put`, and returns everything the call wrote.  Once with put = identity, once per mode with put = the block's guarded copy.
    `oracle(results)`, when given, holds a run to the op's float64 oracle: the normal run always, a guarded run where
    EXCEPTIONS[function, mode] says its sums are ordered differently - then only the results `unordered(name)` selects (all, if
    None) may differ in their bits.  `one_path`: the shape leaves the launcher no choice (H W % 4 != 0), so an ORDER entry does not
    apply and every mode is bit-equal.  `setup()` runs before each run (module-level caches)."""
    name = f"{function}[{case}]" if case else function
    if setup:
        setup()
    ref = fn(_normal)
    torch.cuda.synchronize()
    if oracle is not None:
        oracle(ref)
    for mode in modes:
        kind, why = EXCEPTIONS.get((function, mode), (None, None))
        if one_path and kind == ORDER:
            kind = None
        if setup:
            setup()
        with guarded_allocations(monkeypatch, dev, mode) as block:
            try:
                if kind == "refused":
                    with pytest.raises(RuntimeError, match=why):
                        fn(block.copy)
                    got = None
                else:
                    got = fn(block.copy)
                torch.cuda.synchronize()
            finally:
                _RECORDED.update(block.calls)
        if setup:
            setup()
        if got is None:
            continue
        assert block.allocations, f"{name} [{mode}]: nothing was guarded"
        diff = _differing(ref, got)
        if kind == ORDER:
            assert oracle is not None, f"{name}: an order exception needs the oracle comparison"
            oracle(got)
            print(f"{name} [{mode}]: {ORDER}; {len(diff)} of {len(ref)} results differ in their bits: {_describe(ref, got, diff) or '-'}")
            diff = [k for k in diff if unordered is not None and not unordered(k)]
            assert not diff, f"{name} [{mode}]: differs from the normal call outside the sums: {_describe(ref, got, diff)}"
            continue
        assert kind is None, f"EXCEPTIONS[{function!r}, {mode!r}] = {kind!r} is no permitted kind"
        if diff:
            again = fn(_normal)
            torch.cuda.synchronize()
            unstable = _differing(ref, again)
            assert not unstable, f"{name}: two NORMAL calls differ ({_describe(ref, again, unstable)}): the op is not repeatable"
        assert not diff, f"{name} [{mode}]: differs from the normal call: {_describe(ref, got, diff)}"


def test_device_add_quiets_a_guard_word(dev):
    """What tests/test_guard_selftest.py shows on the host, on the device: a float read-modify-write of a pattern word (here
    torch's in-place add) changes its bits, so an accumulate into a guard is seen although it adds to a NaN."""
    g = guard.Guarded((4,), torch.float32, dev)
    g.assert_intact()
    word = g.parent[g.end:g.end + 4].view(torch.float32)
    before = int(word.view(torch.int32)[0])
    word.add_(0.0)
    after = int(word.view(torch.int32)[0])
    assert before == 0x7FA00000 | ((g.end // 4) & 0xFFFF) and after != before, (hex(before), hex(after))
    side, first, last = g.damage()[0]
    assert side == "after" and 0 <= first <= last <= 3


# ---------------------------------------------------------------------------------------------
# UNet eval plans
# ---------------------------------------------------------------------------------------------
def _eval_fn(dev, variant, sd, inputs, impl, out_slice=False, model=None, extras=False):
    import test_gpu_taps as GT

    def fn(put):
        m = model(dev) if model else GT._model(dev, variant, sd)  # inside a block the weights are guarded inputs too
        eng = m.hip_engine()
        eng.set_impl(impl)
        (x, t, cond, mag), kw = GT._forward_args(dev, variant, inputs)
        kw = {k: put(v) for k, v in kw.items()}
        res, out = {}, None
        if out_slice:  # the tiler's way: a slice of a larger eps buffer
            B, od = x.shape[0], m.out_dim if hasattr(m, "out_dim") else x.shape[1]
            big = torch.full((B + 2, od) + tuple(x.shape[2:]), 7.0, dtype=torch.float32, device=dev)
            out, res["buffer"] = big[1:B + 1], big
        xs, ts, cs = put(x), put(t), None if cond is None else put(cond)
        with torch.no_grad():
            y = eng.forward(xs, ts, cs, mag, reuse_cond=False, out=out, **kw)
        eng.check_faults()
        res["out"] = y
        if extras:  # the entry point without labels on the same plan, and a tap read back from the workspace
            plan = eng._last_plan
            res["x0"] = eng.read_tensor("x0")
            y2 = torch.empty_like(y)
            with torch.cuda.device(dev):
                st = plan.lib.drs_unet_forward(plan.handle, C.c_void_p(plan.packed.data_ptr()), C.c_void_p(xs.data_ptr()),
                                               C.c_void_p(ts.data_ptr()), C.c_void_p(cs.data_ptr()), C.c_void_p(y2.data_ptr()),
                                               C.c_void_p(plan.workspace.data_ptr()), plan.ws_bytes, 0,
                                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            assert st == 0, plan.lib.drs_last_error()
            assert bits_equal(y, y2), "drs_unet_forward and drs_unet_forward_labels differ"
            res["out (drs_unet_forward)"] = y2
        return res
    return fn


EVAL_CASES = [("unaligned", "mfma_bf16x3"), ("edge9", "mfma_bf16x3"), ("mixed", "mfma_bf16x3"), ("sar", "mfma_bf16x3"),
              ("gen", "mfma_bf16x3"), ("mixed", "mfma_f32"), ("mixed", "direct")]


@pytest.mark.parametrize("cid,impl", EVAL_CASES, ids=[f"{c}-{i}" for c, i in EVAL_CASES])
def test_unet_eval_plan(monkeypatch, dev, sds, cid, impl):
    """test_gpu_taps.CASES on the default plan (test_live_taps_of_the_shipped_plan holds every tensor of them to the oracle),
    `mixed` on mfma_f32 (test_live_taps_of_the_fp32_plan) and on direct, which is held to the oracle's output here at the fp32
    bar.  The plan is created inside the block: `packed` and `workspace` are guarded, in `shifted` 8 bytes into their reserve."""
    import taps as T
    import test_gpu_taps as GT
    from conftest import rel_errors
    variant = GT.CASES[cid][0]

    def oracle(res):
        e = rel_errors(res["out"].cpu(), GT._oracle(sds, cid)[T.OUTPUT])
        assert max(e) <= GT.TOL_F32, (cid, impl, e)
    extras = (cid, impl) == ("mixed", "mfma_bf16x3")
    guarded_runs(monkeypatch, dev, "unet_forward", _eval_fn(dev, variant, sds[variant], GT._inputs(cid), impl, extras=extras),
                 oracle if impl == "direct" else None, case=f"{cid},{impl}")


def test_unet_eval_plan_out_slice(monkeypatch, dev, sds):
    """`out=` as the tiler passes it: rows 1 .. B of a larger buffer; the rows around them stay what they were."""
    import test_gpu_taps as GT
    fn = _eval_fn(dev, "superres", sds["superres"], GT._inputs("mixed"), "mfma_bf16x3", out_slice=True)
    ref = fn(_normal)
    assert bool((ref["buffer"][0] == 7.0).all()) and bool((ref["buffer"][-1] == 7.0).all())
    assert ref["out"].data_ptr() == ref["buffer"][1].data_ptr()
    guarded_runs(monkeypatch, dev, "unet_forward", fn, case="out=")


def _ms_eval_case():
    import test_gpu_multispectral as MS
    shape = next(s for s in MS.SHAPES if s[:3] == ("superres", 16, 16))
    variant, cin, cout, B, H, W, mag = shape
    x, t, cond = MS._inputs(f"ms.{variant}.{cin}.{cout}.{H}x{W}", *shape)
    return shape, (x, t, cond, mag)


def test_unet_eval_plan_16_bands(monkeypatch, dev):
    """test_gpu_multispectral.SHAPES at the band limit, 16 -> 16 (test_band_counts_vs_oracle): the stem and projection kernels
    of the few-channel tensors."""
    import test_gpu_multispectral as MS
    (variant, cin, cout, *_), inputs = _ms_eval_case()
    guarded_runs(monkeypatch, dev, "unet_forward",
                 _eval_fn(dev, variant, None, inputs, "mfma_bf16x3", model=lambda d: MS._model(variant, cin, cout, d)[0]), case="16 bands")


# ---------------------------------------------------------------------------------------------
# UNet train step
# ---------------------------------------------------------------------------------------------
def _grads_case(tag):
    """(variant, x, t, cond, noise, mag) of a tests/test_gpu_grads.py case, from its own seeds."""
    import test_gpu_grads as GG
    from diffusionremotesensing_amd import synthetic
    if tag in ("tiny", "single-image"):
        _, B, H, W, mag, ts = next(c for c in GG.SUPERRES_CASES if c[0] == tag)
        return ("superres", synthetic.tensor_normal(f"grads.{tag}.x", (B, 3, H, W)), torch.tensor(ts),
                synthetic.tensor_uniform(f"grads.{tag}.lr", (B, 3, H // mag, W // mag)),
                synthetic.tensor_normal(f"grads.{tag}.noise", (B, 3, H, W)), mag)
    if tag == "sar":  # test_grads_sar
        return ("sar", synthetic.tensor_normal("grads.sar.x", (2, 1, 40, 24)), torch.tensor([GG.T_MAX, 1]),
                synthetic.tensor_uniform("grads.sar.sar", (2, 2, 40, 24)), synthetic.tensor_normal("grads.sar.noise", (2, 1, 40, 24)), 1)
    labels = {"gen-labels": torch.tensor([4, 9, 4]), "gen-unconditional": None}[tag]  # test_grads_generation
    return ("generation", synthetic.tensor_normal("grads.gen.x", (3, 3, 24, 40)), torch.tensor([1, 800, GG.T_MAX]), labels,
            synthetic.tensor_normal("grads.gen.noise", (3, 3, 24, 40)), 1)


def _ms_train_case(bands):
    """test_gpu_multispectral.TRAIN_CASES' superres case at `bands` -> `bands`, as test_train_step_grads feeds it."""
    import test_gpu_multispectral as MS
    from diffusionremotesensing_amd import synthetic
    case = next(c for c in MS.TRAIN_CASES if c[:3] == ("superres", bands, bands))
    variant, cin, cout, B, H, W, mag = case
    tag = f"ms.train.{variant}.{cin}"
    x, _, cond = MS._inputs(tag, *case)
    return case, (variant, x, torch.tensor([1, 1499, 700][:B]), cond, synthetic.tensor_normal(f"{tag}.noise", (B, cout, H, W)), mag)


TRAIN_CASES = ["tiny", "single-image", "sar", "gen-labels", "gen-unconditional", "ms16", "ms13"]


def _train_case(dev, sds, tag):
    """(make_model(device) -> a fresh train-mode model, (variant, x, t, cond, noise, mag), state dict)."""
    import test_gpu_grads as GG
    import test_gpu_multispectral as MS
    if tag.startswith("ms"):
        (variant, cin, cout, *_), batch = _ms_train_case(int(tag[2:]))
        sd = MS._model(variant, cin, cout, "cpu")[1]
        return (lambda d: MS._model(variant, cin, cout, d, train=True)[0]), batch, sd  # (sd: the same seed-0 weights)
    batch = _grads_case(tag)
    sd = sds[batch[0]]
    return (lambda d: GG._model(d, batch[0], sd)), batch, sd


def _train_fn(dev, make_model, batch, impl, patch_engine=None):
    variant, x, t, cond, noise, mag = batch

    def fn(put):
        m = make_model(dev)
        eng = m.hip_engine()
        if impl is not None:
            eng.set_impl(impl, train_impl=impl)
        if patch_engine:
            patch_engine(eng)
        args = (put(x.to(dev)), put(t.to(dev)), None if cond is None else put(cond.to(dev))) + ((mag,) if variant == "superres" else ())
        pred = m(*args)
        loss = F.mse_loss(pred, put(noise.to(dev)))
        loss.backward()
        torch.cuda.synchronize()
        eng.check_faults()
        res = {"pred": pred.detach(), "loss": loss.detach()}
        res.update({f"grad {n}": p.grad for n, p in m.named_parameters()})
        res.update({k: b for k, b in m.named_buffers() if "running_" in k})
        assert sum(v is not None for k, v in res.items() if k.startswith("grad ")) > 100
        return res
    return fn


_ORACLE_GRADS = {}  # case: the float64 step's gradients, computed once and shared by the modes, the impls and the slot test


def _grad_oracle(tag, batch, sd, impl):
    """The float64 step of tests/grad_check.py at the bars tests/test_gpu_grads.py holds `impl` to."""
    import test_gpu_grads as GG
    from grad_check import check_grads, oracle_step
    variant, x, t, cond, noise, mag = batch

    def oracle(res):
        got = {k[5:]: (None if v is None else v.cpu()) for k, v in res.items() if k.startswith("grad ")}
        if tag not in _ORACLE_GRADS:
            _ORACLE_GRADS[tag] = oracle_step(variant, sd, list(got), x, t, cond, noise, mag)[2]
        check_grads(got, _ORACLE_GRADS[tag], *GG._bars(impl), what=f"{tag} [{impl or 'default'}]")
    return oracle


TRAIN_RUNS = [(c, None) for c in TRAIN_CASES] + [("tiny", "direct"), ("tiny", "mfma_bf16x3")]


@pytest.mark.parametrize("tag,impl", TRAIN_RUNS, ids=[f"{c}-{i or 'default'}" for c, i in TRAIN_RUNS])
def test_unet_train_step(monkeypatch, dev, sds, tag, impl):
    """Train-mode forward and loss.backward() inside the block: the train plan's workspace, the packed forward and backward
    images and the flat gradient buffer are guarded, and so are the weights and running statistics the model's layers create on the device.  Every gradient and every
    BatchNorm's running statistics.  Prediction, loss and running statistics equal the unguarded step's bits; the gradients are
    summed with float atomics and differ between two unguarded steps already (EXCEPTIONS), so the unguarded and every guarded
    step's gradients are held to the float64 step of tests/grad_check.py at test_gpu_grads' bars instead.  The cases are
    test_gpu_grads' (`tiny`, `single-image`, SAR, generation with a repeated label and without labels) and
    test_gpu_multispectral.TRAIN_CASES' 16 -> 16 and 13 -> 13; `tiny` also on direct and mfma_bf16x3."""
    make_model, batch, sd = _train_case(dev, sds, tag)
    guarded_runs(monkeypatch, dev, "unet_train_step", _train_fn(dev, make_model, batch, impl), _grad_oracle(tag, batch, sd, impl),
                 case=f"{tag},{impl or 'default'}", unordered=lambda k: k.startswith("grad "))


def _slot_backward(eng, record):
    """`HipUNetEngine.backward` with every gradient in a slot of its own: at least 256 bytes of pattern between neighbours, each
    slot at the address modulo 256 it has in the engine's flat buffer (256-aligned base + 4 * offset), so the same kernels run."""
    from diffusionremotesensing_amd import _lib

    def backward(plan, x, timestep, dout, labels=None):
        sd = eng._tensors(plan.param_names)
        lib = plan.lib
        wanted = [(i, n) for i, n in enumerate(plan.param_names) if sd[n].requires_grad]
        layout, off, cursor = [], 0, 0
        for i, n in wanted:
            k = plan.param_numels[i]
            start = cursor + 256
            start += (4 * off - start) % 256
            layout.append((i, n, start, 4 * k))
            cursor, off = start + 4 * k, off + k
        total = cursor + 256
        g = guard.Guarded((total,), torch.uint8, plan.device, 0, "pattern", "gradient slots")
        ptrs = (C.c_void_p * len(plan.param_names))()
        views = {}
        for i, n, start, nbytes in layout:
            assert (g.view.data_ptr() + start) % 256 == (4 * sum(plan.param_numels[j] for j, _ in wanted if j < i)) % 256
            ptrs[i] = g.view.data_ptr() + start
            views[n] = g.view[start:start + nbytes].view(torch.float32).view_as(sd[n])
        if getattr(plan, "packed_bwd", None) is None:
            plan.packed_bwd_bytes = lib.drs_unet_packed_bwd_bytes(plan.handle)
            plan.packed_bwd = torch.empty(plan.packed_bwd_bytes, dtype=torch.uint8, device=plan.device)
        dout = dout.contiguous()
        head = (plan.handle, C.c_void_p(plan.packed.data_ptr()), C.c_void_p(plan.packed_bwd.data_ptr()), plan.packed_bwd_bytes,
                C.c_void_p(x.data_ptr()), C.c_void_p(timestep.data_ptr()))
        tail = (C.c_void_p(dout.data_ptr()), ptrs, C.c_void_p(plan.workspace.data_ptr()), plan.ws_bytes,
                C.c_void_p(torch.cuda.current_stream(plan.device).cuda_stream))
        with torch.cuda.device(plan.device):
            if labels is None:
                st = lib.drs_unet_backward(*head, *tail)
            else:
                st = lib.drs_unet_backward_labels(*head, C.c_void_p(labels.data_ptr()), int(labels.shape[0]), *tail)
        _lib.check(st, "drs_unet_backward")
        eng._grad_buffer = None
        record.append((g, layout, total))
        return views
    return backward


@pytest.mark.parametrize("tag", TRAIN_CASES)
def test_unet_backward_into_separate_slots(monkeypatch, dev, sds, tag):
    """The engine packs all gradients end to end: a dW that overruns into a neighbour written later is overwritten and the
    element-wise check passes.  Here drs_unet_backward_labels (drs_unet_backward for the cases without labels) writes every
    gradient into its own slot: the gaps keep their pattern, the gradients hold the float64 step's bars like the engine's (they
    are summed with float atomics: EXCEPTIONS), everything else is the engine's step bit for bit."""
    assert EXCEPTIONS["unet_backward_slots", "aligned"][0] == ORDER
    make_model, batch, sd = _train_case(dev, sds, tag)
    ref = _train_fn(dev, make_model, batch, None)(_normal)
    record = []
    with guarded_allocations(monkeypatch, dev, "aligned") as block:
        try:
            got = _train_fn(dev, make_model, batch, None, lambda eng: setattr(eng, "backward", _slot_backward(eng, record)))(block.copy)
        finally:
            _RECORDED.update(block.calls)
    assert len(record) == 1
    g, layout, total = record[0]
    g.assert_intact()
    end, errors = 0, []
    for _, n, start, nbytes in layout + [(None, "the end", total, 0)]:
        try:
            g.assert_pattern(end, start, f"in front of {n}")
        except guard.GuardError as e:
            errors.append(str(e))
        end = start + nbytes
    assert not errors, "\n".join(errors)
    _grad_oracle(tag, batch, sd, None)(got)
    diff = [k for k in _differing(ref, got) if not k.startswith("grad ")]
    assert not diff, _describe(ref, got, diff)
    assert all((ref[k] is None) == (got[k] is None) for k in ref)


# ---------------------------------------------------------------------------------------------
# VGG loss plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl", ["mfma_f32", "mfma_bf16x3"])
@pytest.mark.parametrize("small", ["fewest pixels", "smallest input"])
def test_vgg_loss_plan(monkeypatch, dev, impl, small):
    """Forward and backward of the perceptual loss at the cases of tests/test_gpu_perceptual_layers.py with the fewest pixels
    in the network (40 x 224, no resize) and with the smallest input (24 x 40, resized up: the adjoint of the resize writes a
    small dpred).  The plan (`base256` layout) is created inside the block."""
    import test_gpu_perceptual_layers as PL
    import vgg_oracle as O
    from diffusionremotesensing_amd.perceptual import VGGPerceptualLoss
    case = min(PL.CASES, key=(lambda c: c[0] * (c[1] * c[2] if c[2] == 224 else 224 * 224)) if small == "fewest pixels"
               else (lambda c: c[0] * c[1] * c[2]))
    assert case in ((1, 40, 224, False), (1, 24, 40, False))
    B, H, W, _ = case
    x, y = PL._pair(*case)
    sd = O.seeded_vgg_state_dict()
    monkeypatch.setenv("DRS_VGG_IMPL", impl)

    def fn(put):
        loss_fn = VGGPerceptualLoss(dev, state_dict=sd)
        xd = put(x.to(dev)).requires_grad_(True)
        loss = loss_fn(xd, put(y.to(dev)))
        plan = loss_fn._plan(B, H, W)
        res = {"loss": loss.detach(), "features": plan.read_tensor("features"), "x0": plan.read_tensor("x0")}
        (PL.GRAD_LOSS * loss).backward()
        res["dpred"] = xd.grad
        return res
    guarded_runs(monkeypatch, dev, "vgg_loss", fn, case=f"{impl},{H}x{W}")


# ---------------------------------------------------------------------------------------------
# operators with a *_bytes contract
# ---------------------------------------------------------------------------------------------
def _ragged_conv_cases():
    import test_gpu_parity as GP
    ragged = [c for c in GP.CONV_CASES if c[0] and (c[2] % 2 or c[3] % 2)]  # odd height or width: partial tiles
    assert len(ragged) == 5, ragged
    return ragged


@pytest.mark.parametrize("impl", ["direct", "mfma_f32", "mfma_bf16x3"])
def test_conv2d(monkeypatch, dev, impl):
    """The ragged rows of test_gpu_parity.CONV_CASES (test_conv2d_flavours), with and without the ReLU epilogue."""
    from diffusionremotesensing_amd import hip_ops, synthetic
    for case in _ragged_conv_cases():
        N, Cin, H, W, Cout, k, stride, pad, tr, op = case
        x = synthetic.tensor_normal(f"conv.x.{case}", (N, Cin, H, W))
        w = synthetic.tensor_normal(f"conv.w.{case}", (Cin, Cout, k, k) if tr else (Cout, Cin, k, k), std=(Cin * k * k) ** -0.5)
        b = synthetic.tensor_normal(f"conv.b.{case}", (Cout,), std=0.1)

        def fn(put):
            xd, wd, bd = put(x.to(dev)), put(w.to(dev)), put(b.to(dev))
            return {f"relu={r}": hip_ops.conv2d(xd, wd, bd, stride=stride, padding=pad, transposed=tr, output_padding=op, relu=r,
                                                impl=impl) for r in (False, True)}
        guarded_runs(monkeypatch, dev, "conv2d", fn, case=f"{impl},{case}")


@pytest.mark.parametrize("case", [(3, 32, 32, 9, 17), (1, 128, 64, 24, 40)], ids=lambda c: "x".join(map(str, c)))
def test_upconv_fused(monkeypatch, dev, case):
    """Two of test_gpu_parity.UPFUSE_CASES (test_upconv_fused_matches_convtranspose_cat_conv): the smallest supported heights
    at odd sizes, and ragged tiles on both axes; plain, with the second output, and with the fused projection where that
    test runs it (32 output channels)."""
    import test_gpu_parity as GP
    from diffusionremotesensing_amd import hip_ops, synthetic
    assert case in GP.UPFUSE_CASES
    N, Cc, Ch, LH, LW = case
    h = synthetic.tensor_normal(f"uf.h.{case}", (N, Cc, LH, LW))
    att = synthetic.tensor_normal(f"uf.att.{case}", (N, Ch, 2 * LH, 2 * LW))
    t_w = synthetic.tensor_normal(f"uf.tw.{case}", (Cc, Cc, 3, 3), std=(Cc * 2.25) ** -0.5)
    t_b = synthetic.tensor_normal(f"uf.tb.{case}", (Cc,), std=0.3)
    v_w = synthetic.tensor_normal(f"uf.vw.{case}", (Ch, Cc + Ch, 3, 3), std=((Cc + Ch) * 9) ** -0.5)
    v_b = synthetic.tensor_normal(f"uf.vb.{case}", (Ch,), std=0.3)
    post2 = synthetic.tensor_normal(f"uf.p2.{case}", (N, Ch), std=0.5)
    f_w = synthetic.tensor_normal(f"uf.fw.{case}", (3, 32, 1, 1), std=32 ** -0.5)
    f_b = synthetic.tensor_normal(f"uf.fb.{case}", (3,), std=0.2)

    def fn(put):
        args = [put(t.to(dev)) for t in (h, att, t_w, t_b, v_w, v_b)]
        res = {"y": hip_ops.upconv_fused(*args)}
        res["y (post2)"], res["y2"] = hip_ops.upconv_fused(*args, post2=put(post2.to(dev)))
        if Ch == 32:
            res["projected"] = hip_ops.upconv_fused(*args, fuse_w=put(f_w.to(dev)), fuse_b=put(f_b.to(dev)))
        return res
    guarded_runs(monkeypatch, dev, "upconv_fused", fn, case=str(case))


@pytest.mark.parametrize("which", ["smallest", "groups of four"])
def test_metrics(monkeypatch, dev, which):
    """metrics_pointwise and ssim_mean (through `metrics.image_quality`, one launch of each and the shared workspace) at
    test_gpu_metrics.SHAPES' smallest shape and at its 64 x 64 one, where only the pointers can force the scalar instance;
    every run is held to test_kernels_vs_float64_oracle's bars."""
    import metrics_oracle as MO
    import test_gpu_metrics as GM
    from diffusionremotesensing_amd import metrics
    shape = {"smallest": GM.SHAPES[0], "groups of four": GM.SHAPES[4]}[which]
    assert (shape[2] * shape[3] % 4 == 0) == (which == "groups of four")
    sr, hr = GM._pair(shape, "noise")
    want = MO.image_quality(sr, hr, GM.MAG)
    guarded_runs(monkeypatch, dev, "metrics_pointwise+ssim", lambda put: metrics.image_quality(put(sr.to(dev)), put(hr.to(dev)), GM.MAG),
                 lambda res: GM._assert_matches_oracle(res, want, shape), case=str(shape), unordered=lambda k: k != "ssim",
                 one_path=which == "smallest")


@pytest.mark.parametrize("which", ["smallest", "groups of four"])
def test_ensemble(monkeypatch, dev, which):
    """ensemble_stats / ensemble_scores at test_gpu_ensemble.SHAPES' smallest shape (63 elements) and at (2, 3, 16, 20); every
    run is held to test_maps_and_sums_vs_float64_oracle's bounds."""
    import ensemble_oracle as EO
    import test_gpu_ensemble as GE
    from diffusionremotesensing_amd import hip_ops
    shape = {"smallest": GE.SHAPES[0], "groups of four": GE.SHAPES[1]}[which]
    N, qs, clamp = 3, GE.QUANTILE_LISTS[2], (0.0, 1.0)
    x, y = GE._case(shape, N, "gaussian")
    Mx, Mxy = GE._magnitude(x, None, clamp), GE._magnitude(x, y, clamp)
    stats = EO.statistics(x, qs, clamp)

    def fn(put):
        xd, yd = put(x.to(dev)), put(y.to(dev))
        mean, std, quant = hip_ops.ensemble_stats(xd, qs, clamp)
        sums, hist, crps = hip_ops.ensemble_scores(xd, yd, clamp, crps_map=True)
        return {"mean": mean, "std": std, "quantiles": quant, "sums": sums, "hist": hist, "crps": crps}

    def oracle(res):
        for k in ("mean", "std", "quantiles"):
            GE._map_ratio(res[k], stats[k], Mx, (shape, k))
        GE._map_ratio(res["crps"], EO.crps_map(x, y, clamp), Mxy, (shape, "crps"))
        GE._assert_sums(res["sums"], EO.sums(x, y, clamp), shape)
        assert torch.equal(res["hist"].cpu(), EO.rank_histogram(x, y, clamp))
    guarded_runs(monkeypatch, dev, "ensemble_stats+scores", fn, oracle, case=str(shape), unordered=lambda k: k == "sums",
                 one_path=which == "smallest")


@pytest.mark.parametrize("which", ["odd", "groups of four"])
def test_colorfix(monkeypatch, dev, which):
    """colorfix_adain (a workspace that must be 8-byte aligned: the byte buffers of `shifted` sit at 256 k + 8) at
    test_gpu_colorfix.SHAPES' smallest AdaIN shape / its 64 x 72 one, colorfix_wavelet at 33 x 47 / 64 x 72, 5 levels; every run
    within that module's derived bounds."""
    import colorfix_oracle as CO
    import test_gpu_colorfix as GC
    from diffusionremotesensing_amd import hip_ops
    a_shape, w_shape = {"odd": (GC.SHAPES[1], GC.SHAPES[2]), "groups of four": (GC.SHAPES[3], GC.SHAPES[3])}[which]
    sr, guide = GC._noise(a_shape, 13 + sum(a_shape)), GC._noise(a_shape, 14 + sum(a_shape))
    guarded_runs(monkeypatch, dev, "colorfix_adain", lambda put: {"out": hip_ops.colorfix_adain(put(sr.to(dev)), put(guide.to(dev)))},
                 lambda res: GC._adain_units(res["out"].cpu(), sr, guide) <= GC.ADAIN_UNITS or pytest.fail("adain bound"), case=str(a_shape))
    ws, wg = GC._noise(w_shape, 11 + sum(w_shape)), GC._noise(w_shape, 12 + sum(w_shape))
    want = CO.wavelet(ws, wg, 5)
    guarded_runs(monkeypatch, dev, "colorfix_wavelet", lambda put: {"out": hip_ops.colorfix_wavelet(put(ws.to(dev)), put(wg.to(dev)), 5)},
                 lambda res: GC._wavelet_units(res["out"].cpu(), want, ws, wg) <= GC.WAVELET_UNITS or pytest.fail("wavelet bound"),
                 case=str(w_shape))


def _levels_rotation(lv, n, r):
    return torch.tensor([lv[(i + r) % len(lv)] for i in range(n)])


@pytest.mark.parametrize("which", ["odd", "groups of four"])
def test_prediction_kernels(monkeypatch, dev, which):
    """pred_to_eps_ (into `out` and in place, guided, clipped), noise_v_target and noise_images at test_gpu_prediction.SHAPES'
    (3, 1, 5, 7) and (2, 3, 16, 20), the inputs and level rotation of its kernel tests; x_t of noise_v_target is noise_images'."""
    import test_gpu_prediction as GP
    from diffusionremotesensing_amd import hip_ops
    from oracle import diffusion_oracle as D
    shape = {"odd": GP.SHAPES[1], "groups of four": GP.SHAPES[2]}[which]
    assert (shape[2] * shape[3] % 4 == 0) == (which == "groups of four")
    T = GP.SCHEDULES["cosine"]
    _, ah, _ = D.schedule("cosine", T)
    x, pc, pu, x0 = GP._inputs(shape, 21)
    t = _levels_rotation(GP._levels(T), shape[0], 1)

    def convert(put):
        xd, pcd, pud, td, ahd = (put(a.to(dev)) for a in (x, pc, pu, t, ah))
        res = {}
        for pk in ("eps", "v", "x0"):
            res[f"{pk} out"] = hip_ops.pred_to_eps_(pcd, xd, td, ahd, pk, (0.0, 1.0), out=torch.empty_like(pcd), pred_uncond=pud, cfg_scale=3.0)
            res[f"{pk} in place"] = hip_ops.pred_to_eps_(put(pc.to(dev)), xd, td, ahd, pk, (0.0, 1.0), pred_uncond=pud, cfg_scale=3.0)
            assert bits_equal(res[f"{pk} out"], res[f"{pk} in place"])
        res["pred untouched"] = pcd
        return res
    guarded_runs(monkeypatch, dev, "pred_to_eps_", convert, case=str(shape))

    def targets(put):
        x0d, epsd, td, ahd = (put(a.to(dev)) for a in (x0, pc, t, ah))
        x_t, v = hip_ops.noise_v_target(x0d, epsd, td, ahd)
        return {"x_t": x_t, "v": v}
    guarded_runs(monkeypatch, dev, "noise_v_target", targets, case=str(shape))

    def noised(put):
        x0d, epsd, td, ahd = (put(a.to(dev)) for a in (x0, pc, t, ah))
        out = hip_ops.noise_images(x0d, epsd, td, ahd)
        assert bits_equal(out, hip_ops.noise_v_target(x0d, epsd, td, ahd)[0])  # (test_noise_v_target_kernel_vs_float64_oracle)
        return {"x_t": out}
    guarded_runs(monkeypatch, dev, "noise_images", noised, case=str(shape))


@pytest.mark.parametrize("which", ["odd", "groups of four"])
def test_dynamic_threshold(monkeypatch, dev, which):
    """x0_abs_quantile and pred_to_eps_(x0_threshold=) at test_gpu_threshold.SHAPES' (3, 1, 5, 7) and (2, 3, 16, 20) with the inputs
    of test_threshold_kernel_vs_float64_oracle; the wrapper's cached workspace is dropped so that the block allocates it."""
    import test_gpu_threshold as GT
    from diffusionremotesensing_amd import hip_ops
    from oracle import diffusion_oracle as D
    shape = {"odd": GT.SHAPES[1], "groups of four": GT.SHAPES[2]}[which]
    T = GT.SCHEDULES["cosine"]
    _, ah, _ = D.schedule("cosine", T)
    x, pc, pu = GT._inputs(shape, 41)
    t = _levels_rotation([1, 7, T // 2, T - 1], shape[0], 0)
    p, clip = 0.995, GT.CLIPS[0]

    def fn(put):
        xd, pcd, pud, td, ahd = (put(a.to(dev)) for a in (x, pc, pu, t, ah))
        scales = torch.empty(shape[0], dtype=torch.float32, device=dev)
        eps = hip_ops.pred_to_eps_(pcd, xd, td, ahd, "v", clip, out=torch.empty_like(pcd), x0_threshold=p, scale_out=scales,
                                   pred_uncond=pud, cfg_scale=3.0)
        q = hip_ops.x0_abs_quantile(pcd, xd, td, ahd, "v", clip, p, pred_uncond=pud, cfg_scale=3.0)
        assert bits_equal(q, scales)
        return {"eps": eps, "scales": scales, "quantile": q, "pred untouched": pcd}
    guarded_runs(monkeypatch, dev, "x0_abs_quantile+pred_to_eps_dyn", fn, setup=hip_ops._THRESHOLD_WS.clear, case=str(shape))


def _update_shapes():
    import test_gpu_inpaint as GI
    shapes = sorted({s for s, _ in GI.STEP_CASES}, key=lambda s: -s[0])
    assert [s[2] * s[3] % 4 for s in shapes] == [0, 3], shapes  # (2, 3, 16, 20): groups of four; (1, 1, 7, 9): 63 elements
    return shapes


@pytest.mark.parametrize("which", [0, 1], ids=["groups of four", "odd"])
def test_reverse_step_kernels(monkeypatch, dev, which):
    """sampler_step_, sampler_step_cfg_, ddim_step_, inpaint_step_ (both forms), renoise_ and reverse_step_ at the two shapes of
    test_gpu_inpaint.STEP_CASES, where test_inpaint_step_kernel_vs_float64_oracle holds inpaint_step_ to the oracle and the three
    plain kernels to its unknown branch bit for bit, and test_renoise_kernel_vs_float64_oracle renoise_; dpm_step_ at the 1920-
    and 1027-element tensors of test_dpm_step_kernel_vs_float64_oracle.  In `mixed` the mask sits one byte past a boundary."""
    import test_gpu_dpm as GD
    import test_gpu_inpaint as GI
    from diffusionremotesensing_amd import hip_ops
    from oracle import diffusion_oracle as D
    shape = _update_shapes()[which]
    alpha, ah, beta = D.schedule("cosine", 1500)
    (x, ec, eu, z, known, mask), _ = GI._step_inputs(shape, 1, dev)

    def tables(put):
        return tuple(put(a.to(dev)) for a in (alpha, ah, beta))

    def state(put, *ts):
        return tuple(None if a is None else put(a.to(dev)) for a in ts)

    def sampler(put):
        a, h, b = tables(put)
        xd, ecd, zd = state(put, x, ec, z)
        return {"t=700": hip_ops.sampler_step_(xd, ecd, zd, 700, a, h, b),
                "t=1": hip_ops.sampler_step_(put(x.to(dev)), ecd, None, 1, a, h, b)}
    guarded_runs(monkeypatch, dev, "sampler_step_", sampler, case=str(shape))

    def sampler_cfg(put):
        a, h, b = tables(put)
        xd, ecd, eud, zd = state(put, x, ec, eu, z)
        return {"x": hip_ops.sampler_step_cfg_(xd, ecd, eud, 3.0, zd, 700, a, h, b)}
    guarded_runs(monkeypatch, dev, "sampler_step_cfg_", sampler_cfg, case=str(shape))

    def ddim(put):
        _, h, _ = tables(put)
        xd, ecd, eud, zd = state(put, x, ec, eu, z)
        return {"eta=0.5 guided": hip_ops.ddim_step_(xd, ecd, zd, 49, 42, 0.5, h, eps_uncond=eud, cfg_scale=3.0),
                "eta=0": hip_ops.ddim_step_(put(x.to(dev)), ecd, None, 1499, 1469, 0.0, h)}
    guarded_runs(monkeypatch, dev, "ddim_step_", ddim, case=str(shape))

    def inpaint(put):
        a, h, b = tables(put)
        ecd, eud, zd, kd = state(put, ec, eu, z, known)
        md = put(mask.to(dev), shift=1) if getattr(getattr(put, "__self__", None), "mode", "") == "mixed" else put(mask.to(dev))
        return {"ddim": hip_ops.inpaint_step_(put(x.to(dev)), ecd, zd, kd, md, 49, alpha_hat=h, t_prev=42, eta=0.5, eps_uncond=eud,
                                              cfg_scale=3.0),
                "ancestral": hip_ops.inpaint_step_(put(x.to(dev)), ecd, zd, kd, md, 700, alpha_hat=h, alpha=a, beta=b),
                "to level 0": hip_ops.inpaint_step_(put(x.to(dev)), ecd, None, kd, md, 1, alpha_hat=h, t_prev=0)}
    guarded_runs(monkeypatch, dev, "inpaint_step_", inpaint, case=str(shape))

    def renoise(put):
        _, h, _ = tables(put)
        xd, zd = state(put, x, z)
        return {"x": hip_ops.renoise_(xd, zd, 42, 49, h)}
    guarded_runs(monkeypatch, dev, "renoise_", renoise, case=str(shape))

    def reverse(put):  # the dispatcher, on the guided ancestral move and on the known-pixel DDIM move
        a, h, b = tables(put)
        ecd, eud, zd, kd, md = state(put, ec, eu, z, known, mask)
        return {"ancestral guided": hip_ops.reverse_step_(put(x.to(dev)), ecd, zd, 700, 699, alpha=a, alpha_hat=h, beta=b, eps_uncond=eud,
                                                          cfg_scale=3.0),
                "known ddim": hip_ops.reverse_step_(put(x.to(dev)), ecd, zd, 49, 42, alpha=a, alpha_hat=h, beta=b, ddim=True, eta=0.5,
                                                    known=kd, known_mask=md)}
    guarded_runs(monkeypatch, dev, "reverse_step_", reverse, case=str(shape))

    numel = (1920, 1027)[which]  # test_dpm_step_kernel_vs_float64_oracle's: whole float4 groups; groups and a tail
    dx, dec, deu, dh = (GD._randn(20 + k, (numel,)) for k in range(4))

    def dpm(put):
        _, h, _ = tables(put)
        res = {}
        for tq, t, tp in (GD.MOVES[0], GD.MOVES[2]):  # first order (a history of NaN: only written), second order
            xd, ecd, eud = state(put, dx, dec, deu)
            hd = put(dh.to(dev) if tq is not None else torch.full_like(dh, float("nan")).to(dev))
            hip_ops.dpm_step_(xd, ecd, hd, tq, t, tp, h, eps_uncond=eud, cfg_scale=3.0)
            res[f"x {tq}"], res[f"hist {tq}"] = xd, hd
        return res
    guarded_runs(monkeypatch, dev, "dpm_step_", dpm, case=str(numel))


@pytest.mark.parametrize("which", [3, 4], ids=["rows of 16-byte multiples", "odd rows"])
def test_tile_kernels(monkeypatch, dev, which):
    """gather_tiles, blend_step_ in its four forms and aggregate_tiles with and without known pixels on two of
    test_gpu_tile_chain.GEOMETRIES: 16 x 20 with odd x origins, and 20 x 21, whose rows are no multiple of 16 bytes (the kernel
    tests of test_gpu_tile_chain / test_gpu_dpm / test_gpu_tile_known hold each form to the float64 oracle on both)."""
    import test_gpu_tile_chain as GTC
    from diffusionremotesensing_amd import hip_ops
    from oracle import aggregation_oracle as A
    from oracle import diffusion_oracle as D
    h, w, ps, st, m, Cn = GTC.GEOMETRIES[which]
    assert (w * m % 4 == 0) == (which == 3)
    infos, _ = A.tile_infos(h, w, ps, st, m)
    S, Hs, Ws = ps * m, h * m, w * m
    origins = [(i[0], i[2]) for i in infos]
    wt = A.gaussian_weight(S, S)
    alpha, ah, beta = D.schedule("cosine", 1500)
    x, z, known, hist = (GTC._randn(k, (Cn, Hs, Ws)) for k in (1, 2, 4, 5))
    eps_tiles = GTC._randn(3, (len(infos), Cn, S, S))
    mask = (torch.rand((1, Hs, Ws), generator=torch.Generator().manual_seed(51)) < 0.5).to(torch.uint8)

    def gather(put):
        org = put(hip_ops.tile_origins(origins, S, Hs, Ws, dev))
        scene = put(x.to(dev))
        chunk = torch.full((4, Cn, S, S), float("nan"), dtype=torch.float32, device=dev)
        hip_ops.gather_tiles(scene, org, S, out=chunk, first=max(len(infos) - 2, 0), count=4)  # runs past the last tile
        return {"all": hip_ops.gather_tiles(scene, org, S), "chunk": chunk, "scene untouched": scene}
    guarded_runs(monkeypatch, dev, "gather_tiles", gather, case=str(GTC.GEOMETRIES[which]))

    def blend(put):
        org = put(hip_ops.tile_origins(origins, S, Hs, Ws, dev))
        a, hh, b = (put(t.to(dev)) for t in (alpha, ah, beta))
        ed, wd, zd, kd, md = (put(t.to(dev)) for t in (eps_tiles, wt, z, known, mask))
        unc = torch.zeros(1, dtype=torch.int32, device=dev)
        res = {"ancestral": hip_ops.blend_step_(put(x.to(dev)), ed, org, wd, zd, 700, alpha_hat=hh, alpha=a, beta=b, uncovered=unc),
               "ddim": hip_ops.blend_step_(put(x.to(dev)), ed, org, wd, zd, 49, alpha_hat=hh, t_prev=42, eta=0.5, uncovered=unc)}
        hd = put(hist.to(dev))
        res["dpm"] = hip_ops.blend_step_(put(x.to(dev)), ed, org, wd, None, 49, alpha_hat=hh, t_prev=30, uncovered=unc, hist=hd, t_q=60)
        res["dpm history"] = hd
        res["known ddim"] = hip_ops.blend_step_(put(x.to(dev)), ed, org, wd, zd, 49, alpha_hat=hh, t_prev=42, eta=0.5, uncovered=unc,
                                                known=kd, known_mask=md)
        res["known ancestral"] = hip_ops.blend_step_(put(x.to(dev)), ed, org, wd, zd, 700, alpha_hat=hh, alpha=a, beta=b, uncovered=unc,
                                                     known=kd, known_mask=md)
        res["uncovered"] = unc
        return res
    guarded_runs(monkeypatch, dev, "blend_step_", blend, case=str(GTC.GEOMETRIES[which]))

    def aggregate(put):
        td, wd, kd, md = (put(t.to(dev)) for t in (eps_tiles, wt, known, mask))
        return {"plain": hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws),
                "known": hip_ops.aggregate_tiles(td, origins, wd, Hs, Ws, clamp=(-1.0, 1.0), known=kd, known_mask=md)}
    guarded_runs(monkeypatch, dev, "aggregate_tiles", aggregate, case=str(GTC.GEOMETRIES[which]))


def test_bicubic_and_time_mlp(monkeypatch, dev, seeded_sd):
    """bicubic_upsample at test_gpu_parity.test_bicubic's 7 x 5 and 16 x 16 inputs, time_mlp at test_time_mlp's dim 32."""
    from diffusionremotesensing_amd import hip_ops, synthetic
    for shape, scale in (((1, 3, 7, 5), 2), ((2, 3, 16, 16), 2)):
        x = synthetic.tensor_uniform(f"bicubic.{shape}", shape)
        guarded_runs(monkeypatch, dev, "bicubic_upsample", lambda put: {"y": hip_ops.bicubic_upsample(put(x.to(dev)), scale)}, case=str(shape))
    t = torch.tensor([1, 2, 49, 750, 1499], dtype=torch.int64)
    pfx = "conv_blocks.0.time_mlp"
    guarded_runs(monkeypatch, dev, "time_mlp", lambda put: {"y": hip_ops.time_mlp(put(t.to(dev)), *[
        put(seeded_sd[f"{pfx}.{k}"].to(dev)) for k in ("0.weight", "0.bias", "2.weight", "2.bias")])})


@pytest.mark.parametrize("which", ["odd", "groups of four"])
def test_diffusion_loss_and_timestep_draw(monkeypatch, dev, which):
    """DiffusionLoss (weighted Huber with a table and bins: loss, gradient, per-image losses, partials, bins) at
    test_gpu_loss.SHAPES' (3, 3, 7, 5) and (5, 16, 8, 8), every run held to test_loss_and_grad_vs_oracle_and_torch's bars; the
    timestep draw from rings that the loss launch filled."""
    import test_gpu_loss as GL
    from diffusionremotesensing_amd.losses import DiffusionLoss, LossAwareSampler, LossBins
    shape = {"odd": GL.SHAPES[1], "groups of four": GL.SHAPES[5]}[which]
    import loss_oracle as O
    pred, target, t, table, sample_w = GL._inputs(shape)
    per_image, loss, grad = GL._oracle(shape, "Huber", True)
    nbins, history = 4, 10
    want_bins = O.BinsOracle(GL.T, nbins)
    want_bins.update(per_image, t)

    def fn(put):
        bins = LossBins(GL.T, nbins, dev, history)
        lf = DiffusionLoss("Huber", put(table.to(dev)), bins, delta=GL.DELTA)
        got_loss, got_grad = lf.loss_and_grad(put(pred.to(dev)), put(target.to(dev)), put(t.to(dev)), put(sample_w.to(dev)))
        lf.check_faults()
        return {"loss": got_loss.clone(), "grad": got_grad, "per_image": lf.per_image, "loss_f64": lf.loss_f64.clone(), "bins": bins.buf}

    def oracle(res):
        assert torch.allclose(res["per_image"].cpu(), per_image, rtol=GL.SUM_RTOL, atol=0.0)
        assert abs(res["loss_f64"].item() - loss.item()) <= GL.SUM_RTOL * abs(loss.item())
        assert abs(res["loss"].item() - float(torch.tensor(loss.item(), dtype=torch.float32))) <= GL._ulp32(loss.item())
        GL._assert_grad(res["grad"], grad, f"{shape} Huber weighted")
        buf = res["bins"].cpu()  # include/drs_hip.h: nbins sums, counts, appended, one non-finite count, nbins rings
        words = buf.view(torch.int64)
        assert words[nbins:2 * nbins].tolist() == want_bins.count and int(words[3 * nbins]) == 0
        assert torch.allclose(buf[:nbins], torch.tensor(want_bins.sum, dtype=torch.float64), rtol=GL.SUM_RTOL, atol=0.0)
        rings = buf[3 * nbins + 1:].view(nbins, history)
        for k, appended in enumerate(words[2 * nbins:3 * nbins].tolist()):
            assert appended == len(want_bins.ring[k]) <= history
            assert torch.allclose(rings[k, :appended], torch.tensor(want_bins.ring[k], dtype=torch.float64), rtol=GL.SUM_RTOL, atol=0.0)
    guarded_runs(monkeypatch, dev, "diffusion_loss", fn, oracle, case=str(shape), unordered=lambda k: k != "grad",
                 one_path=which == "odd")
    if which == "odd":
        return
    N = 67
    u = torch.rand(2, N, generator=torch.Generator().manual_seed(2))

    def draw(put):
        bins = LossBins(50, 4, dev)
        GL._fill_rings(dev, bins, O.BinsOracle(50, 4))
        tt, ww = LossAwareSampler(bins).draw(N, put(u.to(dev)))
        return {"t": tt, "w": ww, "bins": bins.buf}
    guarded_runs(monkeypatch, dev, "timestep_draw", draw)


def test_optimizers(monkeypatch, dev):
    """FusedAdam, and FusedAdamW with clipping and decay (the global norm's partials, the device statistics), four steps of
    test_gpu_optim's ragged trajectory (test_trajectory_matches_the_float64_oracle, test_fused_adam_matches_torch_adam): a
    parameter without a gradient, one that skips a step, sizes 1, 5, 81, 4608, 25700 and 70001; parameters, gradients and
    moments are guarded."""
    import test_gpu_optim as GO
    from diffusionremotesensing_amd.optim import FusedAdam, FusedAdamW
    shapes = GO.RAGGED_SHAPES
    host, _ = GO._params(shapes, "cpu")

    def run(put, make):
        params = [torch.nn.Parameter(put(p.clone().to(dev))) for p in host]
        opt = make(params)
        gen = torch.Generator().manual_seed(0)
        for step in range(4):
            for p, g in zip(params, GO._ragged_grads(shapes, step, gen)):
                p.grad = None if g is None else put(g.to(dev))
            opt.step()
        res = {f"p{i}": p.detach() for i, p in enumerate(params)}
        for i, p in enumerate(params):
            for k in ("exp_avg", "exp_avg_sq"):
                res[f"{k}{i}"] = opt.state[p][k] if p in opt.state and opt.state[p] else None
        return opt, res

    def adam(put):
        return run(put, lambda ps: FusedAdam(ps, lr=3e-4))[1]
    guarded_runs(monkeypatch, dev, "FusedAdam", adam)

    def adamw(put):
        opt, res = run(put, lambda ps: FusedAdamW(ps, lr=3e-4, weight_decay=0.01, max_grad_norm=0.05))
        res.update(norm=opt.last_grad_norm(), coef=opt.last_clip_coef(), partials=opt._partials)
        return res
    guarded_runs(monkeypatch, dev, "FusedAdamW", adamw)


def test_ema(monkeypatch, dev, seeded_sd):
    """EMA over two whole UNets (test_ema_multi_tensor_matches_reference_formula): the warm-up copy of parameters and buffers
    and the averaging, one drs_ema_multi launch each; inside a block the tensors the models' layers create on the device are guarded."""
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.UNet_model_superres import EMA, Residual_Attention_UNet_superres

    def fn(put):
        models = []
        for seed in (None, 7, 3):
            m = Residual_Attention_UNet_superres(3, 3, dev)
            m.load_state_dict(seeded_sd if seed is None else synthetic.seeded_state_dict(m.state_dict(), seed))
            models.append(m.to(dev))
        a, b, ema_model = models
        ema_model.eval().requires_grad_(False)
        ema = EMA(0.995)
        ema.step_ema(ema_model, b, step_start_ema=1)  # warm-up: the whole state_dict of b
        copied = {f"copied {k}": v.clone() for k, v in ema_model.state_dict().items()}
        assert all(torch.equal(v, q) for v, q in zip(ema_model.state_dict().values(), b.state_dict().values()))
        ema.step_ema(ema_model, a, step_start_ema=1)
        return dict(copied, **{f"averaged {k}": v for k, v in ema_model.state_dict().items()})
    guarded_runs(monkeypatch, dev, "ema_multi", fn)


def test_feed_gathers(monkeypatch, dev):
    """gather_pairs and gather_u8 at test_gpu_feeds.SHAPES' 5 x 7 rows (35 elements: every row after the first starts unaligned)
    and 8 x 8 rows, five indices with repeats (test_gather_pairs_bit_exact, test_gather_u8_bit_exact)."""
    import test_gpu_feeds as GF
    from diffusionremotesensing_amd.feeds import gather_pairs, gather_u8
    idx = torch.tensor(GF.IDX[5], dtype=torch.int64)
    labels = torch.tensor([7, -3, 2 ** 40 + 5], dtype=torch.int64)
    for pair in (0, 1):
        sar, ndvi = GF._f32_cache(GF.SHAPES[pair], 10 + pair), GF._f32_cache(GF.SHAPES[(pair + 1) % 3], 20 + pair)

        def pairs(put):
            s, n = gather_pairs(put(sar.to(dev)), put(ndvi.to(dev)), put(idx.to(dev)))
            return {"sar": s, "ndvi": n}
        guarded_runs(monkeypatch, dev, "gather_pairs", pairs, case=str(GF.SHAPES[pair]))
        u8 = GF._u8_cache(GF.SHAPES[pair], 30 + GF.SHAPES[pair][0])

        def bytes_(put):
            img, lab = gather_u8(put(u8.to(dev)), put(labels.to(dev)), put(idx.to(dev)))
            return {"img": img, "labels": lab}
        guarded_runs(monkeypatch, dev, "gather_u8", bytes_, case=str(GF.SHAPES[pair]))


@pytest.mark.parametrize("form", ["u8", "u8_f32", "pairs"])
def test_crop_d4(monkeypatch, dev, form):
    """The crop / dihedral kernels at test_gpu_augment.SHAPES' tiny odd case and its all-aligned 16-band one, the 24 items of
    test_crop_d4_bit_exact."""
    import test_gpu_augment as GA
    from diffusionremotesensing_amd.augment import crop_d4_pairs, crop_d4_u8, crop_d4_u8_f32
    for shape in (GA.SHAPES[0], GA.SHAPES[4]):
        c, H, W, S = shape
        items = torch.from_numpy(GA._items(H, W, S))
        sar, ndvi, u8 = GA._f32_cache((2, H, W), 60), GA._f32_cache((1, H, W), 70), GA._u8_cache((c, H, W), 80)
        labels = torch.tensor([7, -3, 2 ** 40 + 5], dtype=torch.int64)

        def fn(put):
            it = put(items.to(dev))
            if form == "pairs":
                return dict(zip(("sar", "ndvi"), crop_d4_pairs(put(sar.to(dev)), put(ndvi.to(dev)), it, S)))
            if form == "u8":
                return {"u8": crop_d4_u8(put(u8.to(dev)), it, S)}
            return dict(zip(("img", "labels"), crop_d4_u8_f32(put(u8.to(dev)), put(labels.to(dev)), it, S)))
        guarded_runs(monkeypatch, dev, f"crop_d4_{form}", fn, case=str(shape))


def test_bsr_kernels(monkeypatch, dev):
    """The blind-degradation kernels at shapes of tests/test_gpu_bsr.py with H W % 4 != 0 and == 0: blur (33 x 47 k = 7, 40 x 72
    k = 25, and a kernel size per image), blur_sep and sharpen (33 x 47, 130 x 200), resize with the quantised copy (33 x 47 ->
    16 x 23, 8 x 8 -> 8 x 8, every mode), noise_ (19 x 23 as test_noise_every_branch_with_given_draws; 20 x 24 is held to its
    oracle and bound here) and the JPEG round trip at JPEG_SHAPES' smallest."""
    import bsr_oracle as BO
    import test_gpu_bsr as GB
    from diffusionremotesensing_amd import bsr
    for shape, k in (GB.BLUR_CASES[2], GB.BLUR_CASES[4]):
        x, ker = GB._rand(shape, 3 + sum(shape), -0.2, 1.2), GB._kernels(shape[0], k, 5 + k)
        guarded_runs(monkeypatch, dev, "bsr.blur", lambda put: {"y": bsr.blur(put(x.to(dev)), put(ker.to(dev)))}, case=f"{shape} k={k}")
    shape = (2, 3, 33, 47)  # test_blur_with_a_kernel_size_per_image
    x, table = GB._rand(shape, 41, -0.2, 1.2), torch.ones((2, 15, 15))
    table[0, 4:11, 4:11], table[1] = GB._kernels(1, 7, 42)[0], GB._kernels(1, 15, 43)[0]
    ksizes = torch.tensor([7, 15], dtype=torch.int32)
    guarded_runs(monkeypatch, dev, "bsr.blur", lambda put: {"y": bsr.blur(put(x.to(dev)), put(table.to(dev)), put(ksizes.to(dev)))},
                 case="kernel sizes")
    for shape in ((2, 3, 33, 47), (1, 3, 130, 200)):
        x = GB._rand(shape, 7 + sum(shape))
        guarded_runs(monkeypatch, dev, "bsr.blur_sep", lambda put: {"y": bsr.blur_sep(put(x.to(dev)), bsr.usm_taps())}, case=str(shape))
        guarded_runs(monkeypatch, dev, "bsr.sharpen", lambda put: {"y": bsr.sharpen(put(x.to(dev)))}, case=str(shape))
    for shape, out in (GB.RESIZE_CASES[0], GB.RESIZE_CASES[3]):
        for mode in (1, 2, 3):
            x = GB._rand(shape, 9 + sum(shape) + mode, -0.2, 1.2)
            guarded_runs(monkeypatch, dev, "bsr.resize", lambda put: dict(zip(("y", "quantised"), bsr.resize(put(x.to(dev)), out[0], out[1], mode,
                                                                                                         quantise=True))), case=f"{shape} {mode}")
    for hw in ((19, 23), (20, 24)):
        n, c = 8, 3
        x = GB._rand((n, c) + hw, 60 + c, -0.1, 1.1)
        z = torch.randn((n, c) + hw, generator=torch.Generator().manual_seed(61))
        mode, par = GB._noise_case(n, c, 62)
        want = BO.noise(x, z, mode, par)

        def oracle(res):
            units = GB._noise_units(x, z, mode, par, res["x"].cpu(), want)
            assert max(units.values()) <= 4, units
        guarded_runs(monkeypatch, dev, "bsr.noise_", lambda put: {"x": bsr.noise_(put(x.to(dev)), put(z.to(dev)), put(mode.to(dev)), put(par.to(dev)))},
                     oracle if hw == (20, 24) else None, case=str(hw))
    n, c = 4, 3  # test_poisson_combination: the gray kind reads its rate plane
    x = GB._rand((n, c, 17, 21), 70)
    mode = torch.tensor([[3, 0], [4, 0], [0, 0], [4, 0]], dtype=torch.int32)
    par = torch.zeros((n, 10))
    par[:, 0] = torch.tensor([150.0, 3000.0, 500.0, 101.5])
    rate = bsr.poisson_rate(x.to(dev), mode.to(dev), par.to(dev)).cpu()
    z = torch.poisson(rate, generator=torch.Generator().manual_seed(71))
    aux = rate[:, 0].contiguous()
    guarded_runs(monkeypatch, dev, "bsr.noise_", lambda put: {"x": bsr.noise_(put(x.to(dev)), put(z.to(dev)), put(mode.to(dev)), put(par.to(dev)),
                                                                            put(aux.to(dev)))}, case="poisson")
    shape = GB.JPEG_SHAPES[0]
    x, q = GB._textured(shape, 80 + shape[2]), torch.tensor([62], dtype=torch.int32)
    guarded_runs(monkeypatch, dev, "bsr.jpeg", lambda put: {"y": bsr.jpeg(put(x.to(dev)), put(q.to(dev)))}, case=str(shape))
    shape = GB.JPEG_SHAPES[3]  # 37 x 53: partial MCUs on both axes
    x, q = GB._textured(shape, 80 + shape[2]), torch.tensor([30], dtype=torch.int32)
    guarded_runs(monkeypatch, dev, "bsr.jpeg", lambda put: {"y": bsr.jpeg(put(x.to(dev)), put(q.to(dev)))}, case=str(shape))


def test_downblur_and_reference_noise(monkeypatch, dev):
    """DownBlur on the Pillow fixtures of test_downblur_matches_pillow_fixtures (all but the 128 x 128 one: 56 x 56 gray, 40 x 24 x4
    -> 6 x 10, 48 x 80, 32 x 32 ...), and the add-noise-and-clip kernel at 5 x 7 and 8 x 8, which is held to x + noise clipped
    to [0, 1] in torch's fp32 here (one exactly rounded sum: the float64 result rounded once)."""
    import numpy as np
    from diffusionremotesensing_amd.degradation import add_noise_clip_, downblur
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degradation_golden.npz")))
    for tag in sorted(k[:-3] for k in g if k.endswith("_hr") and not k.startswith("sq128")):
        hr = g[tag + "_hr"]
        _, _, m, r = g[tag + "_params"]
        planes = torch.from_numpy(np.ascontiguousarray(hr[None] if hr.ndim == 2 else np.moveaxis(hr, -1, 0)))[None]
        guarded_runs(monkeypatch, dev, "downblur", lambda put: dict(zip(("x", "y"), downblur(put(planes.to(dev)), int(m), float(r)))), case=tag)
    for shape in ((2, 3, 5, 7), (2, 3, 8, 8)):
        gen = torch.Generator().manual_seed(5)
        x, noise = torch.rand(shape, generator=gen), 0.3 * torch.randn((shape[0], shape[2], shape[3], shape[1]), generator=gen)

        def oracle(res):
            assert torch.equal(res["x"].cpu(), (x + noise.permute(0, 3, 1, 2)).clamp(0, 1))
        guarded_runs(monkeypatch, dev, "add_noise_clip_", lambda put: {"x": add_noise_clip_(put(x.to(dev)), noise)}, oracle, case=str(shape))


# ---------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------
_SIZE, _PLAN, _NAMES, _PROFILE = ("a size query: host arithmetic", "creates or frees a host-side plan: no device memory is touched",
                                  "reads a name, a shape or a count from the host-side plan",
                                  "profiling: sets a host flag or reads HIP events and host strings")
# Every entry point that launches nothing.  All others must have run inside a guarded block of this module.
NO_DEVICE_WRITE = {
    "drs_last_error": "returns the host-side error string", "drs_abi_version": "returns a constant",
    "drs_x0_threshold_workspace_bytes": _SIZE, "drs_downblur_scratch_bytes": _SIZE, "drs_metrics_workspace_bytes": _SIZE,
    "drs_ensemble_workspace_bytes": _SIZE, "drs_colorfix_adain_workspace_bytes": _SIZE, "drs_bsr_jpeg_scratch_bytes": _SIZE,
    "drs_conv2d_workspace_bytes": _SIZE, "drs_upconv_fused_workspace_bytes": _SIZE, "drs_unet_packed_bytes": _SIZE,
    "drs_unet_workspace_bytes": _SIZE, "drs_unet_packed_bwd_bytes": _SIZE, "drs_vgg_packed_bytes": _SIZE, "drs_vgg_workspace_bytes": _SIZE,
    "drs_unet_plan_create": _PLAN, "drs_unet_plan_destroy": _PLAN, "drs_vgg_plan_create": _PLAN, "drs_vgg_plan_destroy": _PLAN,
    "drs_unet_num_params": _NAMES, "drs_unet_param_name": _NAMES, "drs_unet_param_numel": _NAMES, "drs_unet_num_tensors": _NAMES,
    "drs_unet_tensor_name": _NAMES, "drs_unet_tensor_shape": _NAMES, "drs_vgg_num_tensors": _NAMES, "drs_vgg_tensor_name": _NAMES,
    "drs_vgg_tensor_shape": _NAMES,
    "drs_unet_profile_enable": _PROFILE, "drs_unet_profile_num_ops": _PROFILE, "drs_unet_profile_read": _PROFILE,
    "drs_unet_profile_num_launches": _PROFILE, "drs_unet_profile_launch": _PROFILE, "drs_vgg_profile_enable": _PROFILE,
    "drs_vgg_profile_num_ops": _PROFILE, "drs_vgg_profile_read": _PROFILE,
}


def _cheap_cases(monkeypatch, dev, sds, seeded_sd):
    """One inexpensive parametrisation of every test above (the coverage test run on its own)."""
    test_unet_eval_plan(monkeypatch, dev, sds, "mixed", "mfma_bf16x3")
    for tag in ("tiny", "gen-labels"):  # drs_unet_backward and drs_unet_backward_labels
        test_unet_backward_into_separate_slots(monkeypatch, dev, sds, tag)
    test_vgg_loss_plan(monkeypatch, dev, "mfma_f32", "fewest pixels")
    test_conv2d(monkeypatch, dev, "direct")
    test_upconv_fused(monkeypatch, dev, (3, 32, 32, 9, 17))
    test_metrics(monkeypatch, dev, "smallest")
    test_ensemble(monkeypatch, dev, "smallest")
    test_colorfix(monkeypatch, dev, "odd")
    test_prediction_kernels(monkeypatch, dev, "odd")
    test_dynamic_threshold(monkeypatch, dev, "odd")
    test_reverse_step_kernels(monkeypatch, dev, 1)
    test_tile_kernels(monkeypatch, dev, 4)
    test_bicubic_and_time_mlp(monkeypatch, dev, seeded_sd)
    test_diffusion_loss_and_timestep_draw(monkeypatch, dev, "groups of four")
    test_optimizers(monkeypatch, dev)
    test_ema(monkeypatch, dev, seeded_sd)
    test_feed_gathers(monkeypatch, dev)
    for form in ("u8", "u8_f32", "pairs"):
        test_crop_d4(monkeypatch, dev, form)
    test_bsr_kernels(monkeypatch, dev)
    test_downblur_and_reference_noise(monkeypatch, dev)


def test_every_entry_point_that_launches_is_guarded(monkeypatch, dev, sds, seeded_sd):
    """The entry points of the ABI (`_lib.SIGNATURES`) that no guarded block of this module called are exactly NO_DEVICE_WRITE:
    functions that launch no kernel, copy or memset.  A new entry point is either exercised between guards here or listed there
    with the reason it cannot write (the proxy also records the listed ones a wrapper calls on its way: they are left out of the
    difference).  EXCEPTIONS names only functions and modes that exist."""
    from diffusionremotesensing_amd import _lib
    launching = set(_lib.SIGNATURES) - set(NO_DEVICE_WRITE)
    if launching - _RECORDED:  # run alone: the cheap cases again
        _cheap_cases(monkeypatch, dev, sds, seeded_sd)
    assert set(NO_DEVICE_WRITE) <= set(_lib.SIGNATURES), sorted(set(NO_DEVICE_WRITE) - set(_lib.SIGNATURES))
    assert set(_lib.SIGNATURES) - (_RECORDED - set(NO_DEVICE_WRITE)) == set(NO_DEVICE_WRITE), \
        f"never called inside a guarded block: {sorted(launching - _RECORDED)}"
    assert all(m in MODES and kind in ("refused", ORDER) and why for (_, m), (kind, why) in EXCEPTIONS.items())
