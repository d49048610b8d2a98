"""Every live activation of the plan a user runs against the oracle (tests/taps.py).

`test_unet_blocks_golden` pins 20 taps of a KEEP_ALL plan at 16 x 16: a plan without the composite up-sampling, the fused gates,
the one-launch block 0 or any 16-row-patch kernel - one no user runs.  Here the DEFAULT eval plan (mfma_bf16x3, SP activations,
FL arithmetic, every fusion on) runs on a NaN-poisoned workspace at the smallest shapes that engage each of its forms, and every
named tensor it writes is compared with the oracle, whole and on its four border frames; the launch log ties every op to a
compared tensor, and the kernel instantiations of the five BASELINE configurations to these small cases."""
import json
import os
import subprocess
import sys

import pytest
import torch

import taps as T
from conftest import golden_inputs, rel_errors

pytestmark = pytest.mark.gpu

TOL_BF16X3 = 1e-4  # the bar of the default kernels' taps and forwards (tests/test_gpu_parity.py)
TOL_F32 = 2e-5
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sds(seeded_sd, seeded_sd_sar, seeded_sd_gen):
    return {"superres": seeded_sd, "sar": seeded_sd_sar, "generation": seeded_sd_gen}


# ---------------------------------------------------------------------------------------------
# cases: (variant, batch, H, W, magnification) - the smallest shapes that engage each form (the `*_supported` predicates of
# csrc/), each verified against the launch log below
# ---------------------------------------------------------------------------------------------
CASES = {
    "full": ("superres", 3, 96, 160, 2),       # every fused form at once (inputs of test_unet_forward_rectangular_vs_oracle)
    "edge9": ("superres", 2, 72, 80, 2),       # composite stage 0 at its lower bound (9 x 10 cells), bottleneck with TH just above 8
    "mixed": ("superres", 2, 64, 64, 4),       # bottleneck exactly 8 x 8, stage 0 unfused next to fused stages 1 / 2, x4 conditioning
    "unaligned": ("superres", 1, 88, 104, 2),  # W % 16 = 8: block 0 as dual conv1+skip, no folded projection, no gate_psi
    "trained": ("superres", 2, 128, 128, 2),   # trained-like statistics (test_fl_forward_on_trained_like_statistics)
    "sar": ("sar", 2, 96, 80, 1),              # conditioning at its own resolution, 1 output band
    "gen": ("generation", 5, 64, 96, 1),       # no conditioning tensor, ragged batch, label and unconditional rows mixed
}
GEN_LABELS = [4, -1, 9, 4, 0]


def _inputs(cid):
    from diffusionremotesensing_amd import synthetic
    variant, B, H, W, mag = CASES[cid]
    if cid == "trained":
        x, t, lr = golden_inputs("fl.tl", 2, 2, 3, 128, 2, 1500)
        return x, t, lr, 2
    if cid == "full":
        return (synthetic.tensor_normal("rect.x", (3, 3, 96, 160), 0), synthetic.tensor_randint("rect.t", (3,), 1, 1500, 0),
                synthetic.tensor_uniform("rect.lr", (3, 3, 48, 80), 0), 2)
    t = synthetic.tensor_randint(f"taps.{cid}.t", (B,), 1, 1500)
    if variant == "superres":
        return (synthetic.tensor_normal(f"taps.{cid}.x", (B, 3, H, W)), t,
                synthetic.tensor_uniform(f"taps.{cid}.lr", (B, 3, H // mag, W // mag)), mag)
    if variant == "sar":
        return synthetic.tensor_normal(f"taps.{cid}.x", (B, 1, H, W)), t, synthetic.tensor_uniform(f"taps.{cid}.sar", (B, 2, H, W)), 1
    return synthetic.tensor_normal(f"taps.{cid}.x", (B, 3, H, W)), t, torch.tensor(GEN_LABELS), 1


def _model(dev, variant, sd):
    from diffusionremotesensing_amd.UNet_model_SAR_TO_NDVI import Residual_Attention_UNet_SAR_TO_NDVI
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from diffusionremotesensing_amd.generate_new_imgs.UNet_model_generation import Residual_Attention_UNet_generation
    m = {"superres": lambda: Residual_Attention_UNet_superres(3, 3, dev), "sar": lambda: Residual_Attention_UNet_SAR_TO_NDVI(2, 1, dev),
         "generation": lambda: Residual_Attention_UNet_generation(3, 3, 10, dev)}[variant]()
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _forward_args(dev, variant, inputs):
    """(positional arguments, keyword arguments) of HipUNetEngine.forward for one case."""
    x, t, cond, mag = inputs
    if variant == "generation":
        return (x.to(dev), t.to(dev), None, 1), {"labels": cond.to(dev)}
    return (x.to(dev), t.to(dev), cond.to(dev), mag), {}


def _run(dev, variant, sd, inputs, impl):
    """One case on the device: (output, written tensors, untouched names, launch log of the same forward)."""
    m = _model(dev, variant, sd)
    eng = m.hip_engine()
    eng.set_impl(impl)
    args, kw = _forward_args(dev, variant, inputs)
    with torch.no_grad():
        out, written, untouched = T.live_taps(eng, lambda: eng.forward(*args, reuse_cond=False, **kw))
        _, log = eng.logged_forward(*args, reuse_cond=False, check_weights=False, **kw)
    eng.check_faults()
    return out, written, untouched, log


_ORACLE = {}   # (case, dtype): the CPU oracle's taps, computed once per module
_KERNELS = {}  # case: kernel names (with template arguments) of its default plan's launch log
_TRAINED_SD = {}  # bare_gain: the trained-like state_dict


def _trained_sd(bare_gain):
    """The fixture of test_fl_forward_on_trained_like_statistics, exactly."""
    if bare_gain not in _TRAINED_SD:
        _TRAINED_SD[bare_gain] = _make_trained_sd(bare_gain)
    return _TRAINED_SD[bare_gain]


def _make_trained_sd(bare_gain):
    from diffusionremotesensing_amd import synthetic
    from diffusionremotesensing_amd.UNet_model_superres import Residual_Attention_UNet_superres
    from oracle import unet_oracle as U
    x, t, lr, _ = _inputs("trained")

    def calibrate(sd):
        stats = {}
        with torch.no_grad():
            U.unet_forward(sd, x, t, lr, 2, training=True, stats=stats)
        return {bn: ((rm - 0.9 * sd[bn + ".running_mean"]) / 0.1, (rv - 0.9 * sd[bn + ".running_var"]) / 0.1)
                for bn, (rm, rv) in stats.items()}
    return synthetic.trained_like_state_dict(Residual_Attention_UNet_superres(3, 3, "cpu").state_dict(), calibrate, seed=3,
                                             bare_gain=bare_gain)


def _case_sd(sds, cid, bare_gain=1.0):
    return _trained_sd(bare_gain) if cid == "trained" else sds[CASES[cid][0]]


def _oracle(sds, cid, dtype=torch.float32, bare_gain=1.0):
    key = (cid, dtype, bare_gain)
    if key not in _ORACLE:
        _ORACLE[key] = T.oracle_taps(CASES[cid][0], _case_sd(sds, cid, bare_gain), _inputs(cid), dtype)
    return _ORACLE[key]


def _by_op(log):
    by_op = {}
    for op, k in log:
        by_op.setdefault(op, []).append(k)
    return by_op


def _assert_kernels(log, expected, absent_ops=()):
    """{op: substring of a kernel name that op must have launched}, and ops that must not be in the log."""
    by_op = _by_op(log)
    for op, sub in expected.items():
        assert any(sub in k for k in by_op.get(op, [])), f"{op}: expected {sub}, launched {by_op.get(op)}; ops: {sorted(by_op)}"
    for op in absent_ops:
        assert op not in by_op, f"{op} ran ({by_op[op]}): this case is meant for the plan without it"


def _check_case(cid, out, written, untouched, log, want, tol, compared_literal):
    """The four checks every case makes; returns compare's table."""
    e_max, e_l2 = rel_errors(out, want[T.OUTPUT])
    print(f"{cid}: output max-rel {e_max:.2e} rel-L2 {e_l2:.2e}; {len(written)} tensors written, {len(untouched)} untouched")
    out_tol = tol if not isinstance(tol, dict) else tol[""]
    compared = {n for n in written if n in want}
    table, _ = T.compare(written, want, tol)
    T.assert_within(table, cid)  # (first: it names the layers; the output bar below is the anchor other tests hold too)
    assert e_max <= out_tol and e_l2 <= out_tol, f"{cid} output: max-rel {e_max:.3e} rel-L2 {e_l2:.3e}"
    assert compared == compared_literal, (f"{cid}: compared set changed: no longer compared {sorted(compared_literal - compared)}, "
                                          f"new {sorted(compared - compared_literal)}; written without a reference "
                                          f"{sorted(set(written) - compared)}")
    assert not set(written) - compared, f"{cid}: written tensors without a reference: {sorted(set(written) - compared)}"
    T.check_ops(log, compared, set(written))
    return table


# ---------------------------------------------------------------------------------------------
# what each case's default plan materialises (recorded from the device, reviewed against csrc/unet_forward.hip)
# ---------------------------------------------------------------------------------------------
# Common to every SP plan: the conditioning branch's three named tensors, x0, each ResConvBlock's h and output (the shortcut
# rides inside conv2 as K-chunks: `.shortcut` never exists), the three downs, each stage's input x + temb and its ups.i.conv.
_ENCODER = {"x0", "conv_blocks.0", "conv_blocks.1.h", "conv_blocks.1", "conv_blocks.2.h", "conv_blocks.2", "bottle_neck.h",
            "downs.0", "downs.1", "downs.2"}
_STAGES = {"ups.0.in", "ups.1.in", "ups.2.in", "ups.0.conv", "ups.1.conv", "ups.2.conv"}
_LR = {"LR_encoder", "upsampled_lr_img", "cond"}
_GATED = {"attention_blocks.0", "attention_blocks.1", "attention_blocks.2.psi"}
_ATT_HALVES = {"up_convs.0.att_half", "up_convs.1.att_half"}
# `full`: block 0 in one launch (conv_blocks.0.h stays in LDS).  Every stage input exists ONLY as ups.i.in (xt_only: the
# bottleneck's conv2 and the composites of stages 0 / 1 write x + temb and nothing else, so bottle_neck, up_convs.0 and
# up_convs.1 are not materialised).  Composite stages never write ups.i (cat.i[:, :Cc]); stages 0 / 1 keep the att-half's partial
# sums, stage 2 hands its own over through the output tensor.  gate_psi: the top gate stops at psi, attention_blocks.2 never
# exists.  The fused gates keep g, g1, relu (and psi of stages 0 / 1) on chip.
_FULL = _LR | _ENCODER | _STAGES | _GATED | _ATT_HALVES
# stage 0 as ConvTranspose + up_conv over cat.0 (LH = 8 declines the composite): ups.0, hence all of cat.0, and up_convs.0
# exist, no att-half; the bottleneck's 8-row kernels decline the x + temb-only form, so bottle_neck is written next to ups.0.in
_STAGE0_UNFUSED = (_FULL - {"up_convs.0.att_half"}) | {"bottle_neck", "cat.0", "ups.0", "up_convs.0"}
COMPARED = {
    "full": _FULL,
    "edge9": _FULL,
    "mixed": _STAGE0_UNFUSED,
    # block 0 as the dual conv1+skip launch and conv2: conv_blocks.0.h exists (the skip tensor does not); no gate_psi: the top
    # gate writes attention_blocks.2 into cat.2 and no psi
    "unaligned": (_FULL - {"attention_blocks.2.psi"}) | {"attention_blocks.2", "conv_blocks.0.h"},
    # the encoded SAR image is used at its own resolution: upsampled_lr_img is not written
    "sar": (_FULL - {"LR_encoder", "upsampled_lr_img"}) | {"SAR_encoder"},
    # no conditioning branch; 8 x 12 bottleneck: stage 0 unfused as in `mixed`
    "gen": _STAGE0_UNFUSED - _LR,
}
# mfma_f32: fp32 channels-last activations, nothing fused but the shortcut (K-chunks of conv2: `.shortcut` never exists) and the
# output projection (epilogue of up_convs.2, whose 32-channel tensor is then not written)
_F32 = _LR | _ENCODER | {"conv_blocks.0.h", "conv_blocks.0.skip", "bottle_neck", "up_convs.0", "up_convs.1"} | {
    f"{n}.{i}{leaf}" for i in range(3) for n, leaf in (("gating_signals", ""), ("attention_blocks", ""), ("attention_blocks", ".g1"),
                                                        ("attention_blocks", ".relu"), ("attention_blocks", ".psi"), ("ups", ""),
                                                        ("ups", ".conv"), ("cat", ""))}
COMPARED_F32 = {"full": _F32, "mixed": _F32}

_FUSED_TOP = {"attention_gate.2": "attn_gate_sp_kernel<2, true>",  # PSI_ONLY
              "up_convs.2.att": "conv3x3_proj_sp_kernel<true>",    # ah_proj + gate_psi: reads the skip tensor, gated by psi
              "up_convs.2.fused": "upfuse_proj_sp_kernel"}         # uf_proj
KERNELS = {
    "full": dict(_FUSED_TOP, **{
        "conv_blocks.0.fused": "resblock0_kernel", "downs.0": "down_sp_kernel", "downs.1": "conv_s2_sp_kernel",
        "conv_blocks.1.conv1.0": "tapconv_fl_kernel<false>", "conv_blocks.2.conv2.0": "tapconv_fl_kernel<true>",
        "bottle_neck.conv2.0": "tapconv_fl_kernel<true>", "attention_gate.0": "attn_gate_wide2_kernel",
        "attention_gate.1": "attn_gate_sp_kernel<4, false>", "up_convs.0.edges": "upfuse_edges_mfma_kernel",
        "up_convs.0.att": "tapconv_fl_kernel", "up_convs.0.fused": "upfuse_sp_kernel<false>",
        "up_convs.1.att": "tapconv_fl_kernel", "up_convs.1.fused": "upfuse_sp_kernel<false>"}),
    # 9 x 10 cells: the composite's lower bound; the bottleneck's 16-row patches (TH just above 8) run the wave-specialised
    # kernel in its FL form (tapconv_fl_kernel: what the default plan puts on every 64-channel-per-item 3x3 layer).  OW = 40 is
    # no multiple of down_sp's patch: downs.0 on conv_s2_sp.
    "edge9": dict(_FUSED_TOP, **{
        "up_convs.0.fused": "upfuse_sp_kernel<false>", "up_convs.0.att": "tapconv_fl_kernel",
        "bottle_neck.conv1.0": "tapconv_fl_kernel<false>", "bottle_neck.conv2.0": "tapconv_fl_kernel<true>",
        "ups.0.conv": "tapconv_fl_kernel", "downs.0": "conv_s2_sp_kernel", "conv_blocks.0.fused": "resblock0_kernel"}),
    "mixed": dict(_FUSED_TOP, **{
        "bottle_neck.conv1.0": "tapconv_sp8_kernel<false>", "bottle_neck.conv2.0": "tapconv_sp8_kernel<true>",
        "ups.0.conv": "tapconv_sp8_kernel<false>", "ups.0.transform": "tapconv_mfma_kernel<PolicyBF16X3",
        "up_convs.0": "tapconv_fl_kernel", "up_convs.1.fused": "upfuse_sp_kernel<false>", "lr_branch": "bicubic_kernel"}),
    "unaligned": {
        "conv_blocks.0.conv1.0+skip": "tapconv_sp_kernel<false, 64", "conv_blocks.0.conv2.0": "tapconv_sp_kernel<true, 32",
        "downs.0": "conv_s2_sp_kernel", "attention_gate.2": "attn_gate_sp_kernel<2, false>",
        "up_convs.2.att": "tapconv_sp_kernel<false, 32, true",  # the fuse_w epilogue of the att-half
        "up_convs.2.fused": "upfuse_sp_kernel<true>"},          # the non-folded composite with the projection epilogue
    "sar": dict(_FUSED_TOP, **{"conv_blocks.0.fused": "resblock0_kernel", "lr_branch": "stem_kernel<16>",
                               "up_convs.0.fused": "upfuse_sp_kernel<false>"}),
    # 8 x 12 bottleneck: neither the 8 x 8 instance nor 16-row patches: the lock-step kernel, and x + temb of stage 0 from a pass
    # of its own (plan_conv: split_out2)
    "gen": dict(_FUSED_TOP, **{"bottle_neck.conv1.0": "tapconv_mfma_kernel<PolicyBF16X3", "bottle_neck.conv2.0": "sp_add_rowvec_kernel",
                               "ups.0.transform": "tapconv_mfma_kernel<PolicyBF16X3", "up_convs.0": "tapconv_fl_kernel",
                               "conv_blocks.0.fused": "resblock0_kernel", "downs.0": "down_sp_kernel"}),
}
_COMPOSITE0 = ("up_convs.0.edges", "up_convs.0.att", "up_convs.0.fused")
ABSENT_OPS = {"full": ("ups.0.transform", "up_convs.0"), "edge9": ("ups.0.transform", "up_convs.0"), "mixed": _COMPOSITE0,
              "unaligned": ("conv_blocks.0.fused",), "gen": _COMPOSITE0 + ("lr_branch",)}


# what `full` must keep comparing whatever else changes: one tensor per layer of the fused plan
FULL_AT_LEAST = {"x0", "conv_blocks.0", "conv_blocks.1.h", "conv_blocks.1", "conv_blocks.2.h", "conv_blocks.2", "bottle_neck.h",
                 "downs.0", "downs.1", "downs.2", "ups.0.conv", "ups.1.conv", "ups.2.conv", "ups.0.in", "ups.1.in", "ups.2.in",
                 "attention_blocks.0", "attention_blocks.1", "attention_blocks.2.psi", "up_convs.0.att_half", "up_convs.1.att_half",
                 "LR_encoder", "upsampled_lr_img"}
assert FULL_AT_LEAST <= COMPARED["full"]

SEEDED = ["full", "edge9", "mixed", "unaligned", "sar", "gen"]


@pytest.mark.parametrize("cid", SEEDED)
def test_live_taps_of_the_shipped_plan(dev, sds, cid):
    variant = CASES[cid][0]
    out, written, untouched, log = _run(dev, variant, sds[variant], _inputs(cid), "mfma_bf16x3")
    _KERNELS[cid] = {k for _, k in log}
    _assert_kernels(log, KERNELS[cid], ABSENT_OPS.get(cid, ()))
    _check_case(cid, out, written, untouched, log, _oracle(sds, cid), TOL_BF16X3, COMPARED[cid])


@pytest.mark.parametrize("cid", ["full", "mixed"])
def test_live_taps_of_the_fp32_plan(dev, sds, cid):
    """The same inputs under mfma_f32: a plan with fp32 channels-last activations and no fused form (five-launch gates,
    ConvTranspose + up_conv pairs), at sizes where it is not tiny, held to the fp32 bar."""
    variant = CASES[cid][0]
    out, written, untouched, log = _run(dev, variant, sds[variant], _inputs(cid), "mfma_f32")
    assert not any(op.endswith((".fused", ".att", ".edges", "+skip")) or op.startswith("attention_gate") for op, _ in log)
    _check_case(cid + " (mfma_f32)", out, written, untouched, log, _oracle(sds, cid), TOL_F32, COMPARED_F32[cid])


# ---------------------------------------------------------------------------------------------
# trained-like statistics: per-layer error of the FL arithmetic against the float64 oracle
# ---------------------------------------------------------------------------------------------
# A tap passes inside 1e-4.  Above it, it is accepted only where the FL error is within 3x the pure split-bf16 error
# (DRS_FL=0, own process: the switch is read once) of the same entry and norm - the FL design claims the same 16-bit operand
# mantissa, so a larger ratio is an FL defect and not conditioning - and then holds 2x its measured value:
#   {bare_gain: {(tensor, frame): bar}}       measured FL (max-rel)   split bf16   ratio
TRAINED_BARS = {
    1.0: {("attention_blocks.2.psi", "all"): 2 * 1.36e-4,   # 1.36e-4                6.53e-5      2.1
          ("up_convs.0.att_half", "row-1"): 2 * 1.14e-4},   # 1.14e-4                5.14e-5      2.2
    300.0: {("attention_blocks.0", "all"): 2 * 1.09e-4,     # 1.09e-4                6.27e-5      1.7
            ("attention_blocks.2.psi", "all"): 2 * 1.35e-4},  # 1.35e-4              6.99e-5      1.9
}
FL_RATIO = 3.0
_SPLIT_BF16 = {}  # bare_gain: {"tensor[frame]": [max-rel, rel-L2]} of the DRS_FL=0 plan, from the child process


def _trained_run(dev, bare_gain):
    """(output, written, untouched, log, float64 oracle taps) of the trained-like case in THIS process's arithmetic."""
    sd = _trained_sd(bare_gain)
    want = _oracle(None, "trained", torch.float64, bare_gain)
    return _run(dev, "superres", sd, _inputs("trained"), "mfma_bf16x3") + (want,)


def _dump_split_bf16_errors():
    """Child process (DRS_FL=0): one JSON line with every tap's errors on the split-bf16 kernels, both gains."""
    assert os.environ.get("DRS_FL") == "0"
    from diffusionremotesensing_amd import _lib
    _lib.load()
    res = {}
    for gain in TRAINED_BARS:
        out, written, _, log, want = _trained_run(torch.device("cuda:0"), gain)
        assert not any("tapconv_fl_kernel" in k for _, k in log), "DRS_FL=0 did not switch the FL kernels off"
        table, _ = T.compare(written, want, 1.0)
        res[str(gain)] = {f"{n}[{fr}]": [a, b] for n, fr, a, b, _ in table}
    print("SPLIT_BF16 " + json.dumps(res))


def _split_bf16_errors():
    if not _SPLIT_BF16:
        code = f"import sys; sys.path[:0] = [{HERE!r}, {os.path.dirname(HERE)!r}]; import test_gpu_taps as G; G._dump_split_bf16_errors()"
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DRS_FL="0"), capture_output=True, text=True,
                           timeout=300, cwd=os.path.dirname(HERE))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("SPLIT_BF16 ")]
        assert r.returncode == 0 and lines, r.stdout[-2000:] + r.stderr[-2000:]
        _SPLIT_BF16.update({float(g): v for g, v in json.loads(lines[-1][len("SPLIT_BF16 "):]).items()})
    return _SPLIT_BF16


@pytest.mark.parametrize("bare_gain", [1.0, 300.0])
def test_live_taps_on_trained_like_statistics(dev, bare_gain):
    """The fixture of test_fl_forward_on_trained_like_statistics (2 x 128 x 128; running_var down to 1e-3, gamma up to 10;
    bare_gain 300: FL inputs in the thousands), every live tensor against the oracle run in float64.  Only the output was held
    before (7.8e-5 of 1e-4).  Measured on an MI355X (FL / split bf16, worst entry): gain 1: 1.36e-4 / 8.8e-5, gain 300: 1.35e-4 /
    7.0e-5 max-rel; rel-L2 stays under 8.5e-5 / 4e-5 everywhere."""
    out, written, untouched, log, want = _trained_run(dev, bare_gain)
    _KERNELS.setdefault("trained", set()).update(k for _, k in log)
    assert sum("tapconv_fl_kernel" in k for _, k in log) >= 8, "the FL kernel did not run"
    bars = dict(TRAINED_BARS[bare_gain])
    bars[""] = TOL_BF16X3
    table = _check_case(f"trained (gain {bare_gain})", out, written, untouched, log, want, bars, COMPARED["full"])
    above = [r for r in table if max(r[2], r[3]) > TOL_BF16X3]
    assert {(r[0], r[1]) for r in above} <= set(TRAINED_BARS[bare_gain])
    if above:
        split = _split_bf16_errors()[bare_gain]
        for name, frame, e_max, e_l2, _ in above:
            s_max, s_l2 = split[f"{name}[{frame}]"]
            print(f"  {name}[{frame}]: FL {e_max:.2e} / {e_l2:.2e}, split bf16 {s_max:.2e} / {s_l2:.2e}")
            for fl, sp, norm in ((e_max, s_max, "max-rel"), (e_l2, s_l2, "rel-L2")):
                assert fl <= TOL_BF16X3 or fl <= FL_RATIO * sp, (f"{name}[{frame}] {norm}: FL {fl:.2e} is more than {FL_RATIO} x the split-bf16 "
                                                                 f"error {sp:.2e} of the same tap: an FL defect, not conditioning")


def _log_only(dev, sd, variant, inputs):
    m = _model(dev, variant, sd)  # (the engine holds its module weakly)
    eng = m.hip_engine()
    eng.set_impl("mfma_bf16x3")
    args, kw = _forward_args(dev, variant, inputs)
    with torch.no_grad():
        eng.forward(*args, reuse_cond=False, **kw)
        _, log = eng.logged_forward(*args, reuse_cond=False, check_weights=False, **kw)
    eng.check_faults()
    return {k for _, k in log}


# {kernel name: reason} of kernels that write no activation (pack, layout conversion, gate_bias) and may therefore run at a
# production shape without a tap case.  Empty: every kernel of the five production logs, gate_bias_kernel included, is launched
# by a case above as well.
NO_ACTIVATION_KERNELS = {}


def test_every_production_kernel_is_tap_checked(dev, sds):
    """The kernel instantiations (names with template arguments) the five BASELINE eval shapes launch are a subset of those
    the tap cases above launched: a new instantiation cannot ship having been compared only at full size, on the output."""
    from diffusionremotesensing_amd import synthetic
    for cid in SEEDED + ["trained"]:
        if cid not in _KERNELS:  # (run alone: the launch logs of the cases, without their oracles)
            _KERNELS[cid] = _log_only(dev, _case_sd(sds, cid), CASES[cid][0], _inputs(cid))
    covered = set().union(*_KERNELS.values())

    def sr(B, S):
        return "superres", (synthetic.tensor_normal("prod.x", (B, 3, S, S)), synthetic.tensor_randint("prod.t", (B,), 1, 1500),
                            synthetic.tensor_uniform("prod.lr", (B, 3, S // 2, S // 2)), 2)
    production = {
        "configs[0] 4 x 128^2 x2": sr(4, 128),
        "configs[1] 16 x 256^2 x2": sr(16, 256),
        "configs[3] SAR 32 x 128^2": ("sar", (synthetic.tensor_normal("prod.sx", (32, 1, 128, 128)), synthetic.tensor_randint("prod.t", (32,), 1, 1000),
                                              synthetic.tensor_uniform("prod.sar", (32, 2, 128, 128)), 1)),
        "configs[4] generation 64 x 64^2": ("generation", (synthetic.tensor_normal("prod.gx", (64, 3, 64, 64)), synthetic.tensor_randint("prod.t", (64,), 1, 1000),
                                                           torch.arange(64) % 10, 1)),
        "n = 1 at 256^2": sr(1, 256),
    }
    missing = {}
    for what, (variant, inputs) in production.items():
        for k in _log_only(dev, sds[variant], variant, inputs) - covered:
            if k not in NO_ACTIVATION_KERNELS:
                missing.setdefault(k, []).append(what)
    assert not missing, "kernels no tap case launches: " + "; ".join(f"{k} ({', '.join(v)})" for k, v in sorted(missing.items()))
