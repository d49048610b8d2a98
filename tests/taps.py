"""Per-layer comparison of the plan a user runs (default eval plan: SP activations, FL arithmetic, every fusion on) with the
oracle (a plain module, imported by tests/test_gpu_taps.py and tests/test_taps_selftest.py).

`live_taps` poisons the workspace with NaN bit patterns, runs one forward and sorts every named tensor of the plan into
written / untouched (a half-written one is a finding); `oracle_taps` returns the oracle's taps plus the references of the
tensors the shipped plan materialises and the oracle does not name (all computed on the CPU from oracle taps and the
state_dict); `compare` holds every live tensor, and its four one-pixel border frames on their own scale, to a bar.
`OP_WRITES` ties every op of the launch log to the named tensors it may write, so that a case cannot go hollow."""
import torch
import torch.nn.functional as F

from conftest import rel_errors

OUTPUT = "<output>"  # the network's output tensor (the caller's, not a workspace tensor)

# channel counts of the decoder stages (oracle.unet_oracle.UP): stage i reads Cc = UP[i] channels and writes Ch = UP[i + 1]
UP = (256, 128, 64, 32, 16)

# concat buffers: a tensor whose channel slices are named tensors of their own.  A composite stage writes only the attention
# slice (the up-sampled slice never exists), so the buffer as a whole is judged through its slices.
CONTAINERS = {f"cat.{i}": (f"ups.{i}", f"attention_blocks.{i}") for i in range(3)}


def _op_writes():
    """{op of the launch log: names of the tensors it may write}.  () = an op whose result never exists as a named tensor."""
    w = {
        "time_mlp": (),  # the embedding table: no named tensor
        "lr_branch": ("LR_encoder", "SAR_encoder", "upsampled_lr_img", "cond"),  # (its interior ping-pong buffers are unnamed)
        "conv0": ("x0",),
        "conv_blocks.0.fused": ("conv_blocks.0",),  # the one-launch block 0: h stays in LDS
        "output": (OUTPUT,),
    }
    for i, blk in enumerate(("conv_blocks.0", "conv_blocks.1", "conv_blocks.2", "bottle_neck")):
        w[blk + ".conv1.0"] = (blk + ".h",)
        w[blk + ".conv1.0+skip"] = (blk + ".h",)
        w[blk + ".shortcut_conv.0"] = (blk + ".shortcut",)
        # the bottleneck's conv2 also writes x + temb of decoder stage 0 (TapConv::out2), and only that when both readers take it
        w[blk + ".conv2.0"] = (blk,) if i < 3 else (blk, "ups.0.in")
        if i < 3:
            w[f"downs.{i}"] = (f"downs.{i}",)
    for skip in ("conv_upsampled_lr_img", "conv_SAR_img", "conv_skip"):
        w["conv_blocks.0." + skip] = ("conv_blocks.0.skip",)
    for i in range(3):
        a = f"attention_blocks.{i}"
        w[f"attention_gate.{i}"] = (a, a + ".psi")  # fused gate: att into cat.i, or psi alone (DecStage::gate_psi)
        w[f"gating_signals.{i}.conv"] = (f"gating_signals.{i}",)
        w[a + ".w_g.0"] = (a + ".g1",)
        w[a + ".w_x.0"] = (a + ".relu",)
        w[a + ".psi.0"] = (a + ".psi",)
        w[a + ".result.0"] = (a,)
        w[f"ups.{i}.conv"] = (f"ups.{i}.conv",)
        for ph in ("", ".phase0", ".phase1", ".phase2", ".phase3"):
            w[f"ups.{i}.transform{ph}"] = (f"ups.{i}",)
        nxt = (f"up_convs.{i}", f"ups.{i + 1}.in") if i < 2 else ("up_convs.2", OUTPUT)
        w[f"up_convs.{i}"] = nxt
        w[f"up_convs.{i}.edges"] = ()  # edge vectors: unnamed workspace
        w[f"up_convs.{i}.att"] = (f"up_convs.{i}.att_half",) if i < 2 else ()  # stage 2: projected, into the output
        w[f"up_convs.{i}.fused"] = nxt if i < 2 else ()  # stage 2: adds its part to the output
    return w


OP_WRITES = _op_writes()


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
def classify(t):
    """'untouched' (every element NaN), 'written' (none) or 'partial'."""
    nan = torch.isnan(t)
    if bool(nan.all()):
        return "untouched"
    return "partial" if bool(nan.any()) else "written"


def nan_box(t):
    """Bounding box [(first, last)] per dimension of the NaN elements of `t`."""
    idx = torch.isnan(t).nonzero()
    return [(int(idx[:, d].min()), int(idx[:, d].max())) for d in range(t.dim())]


def poison_workspace(eng):
    """The recipe of test_forward_reads_nothing_it_did_not_write: every word of the workspace 0xFFFFFFFF (an fp32 NaN, and two
    bf16 NaNs of an SP pixel)."""
    ws = eng._last_plan.workspace
    ws.view(torch.int32)[: ws.numel() // 4].fill_(-1)


def sort_tensors(tensors):
    """({name: tensor} of the written ones, sorted names of the untouched ones); raises AssertionError on a partial tensor
    that is not a concat buffer judged through its slices.  A concat buffer is live only when all its slices are."""
    written, untouched, partial = {}, [], []
    kinds = {name: classify(t) for name, t in tensors.items()}
    for name, t in tensors.items():
        kind = kinds[name]
        if name in CONTAINERS and all(kinds.get(v) in ("written", "untouched") for v in CONTAINERS[name]):
            kind = "written" if all(kinds[v] == "written" for v in CONTAINERS[name]) else "untouched"
        if kind == "written":
            written[name] = t
        elif kind == "untouched":
            untouched.append(name)
        else:
            partial.append(f"{name} {tuple(t.shape)}: NaN inside {nan_box(t)}")
    assert not partial, "half-written activations: " + "; ".join(partial)
    return written, sorted(untouched)


def live_taps(eng, forward_fn):
    """`forward_fn()` runs one forward of `eng` with reuse_cond=False and returns its output.  Returns (output, {name: NCHW
    tensor on the host} of every named tensor that forward wrote, names it left alone)."""
    forward_fn()  # plan and packed weights in place
    poison_workspace(eng)
    out = forward_fn()
    torch.cuda.synchronize()
    tensors = {name: eng.read_tensor(name).cpu() for name in eng.tensor_names()}
    written, untouched = sort_tensors(tensors)
    return out.cpu(), written, untouched


# ---------------------------------------------------------------------------------------------
# oracle side
# ---------------------------------------------------------------------------------------------
def _names(variant):
    """(conditioning encoder, conditioning convolution / block-0 skip convolution) of a variant."""
    return {"superres": ("LR_encoder", "conv_upsampled_lr_img"), "sar": ("SAR_encoder", "conv_SAR_img"),
            "generation": (None, "conv_skip")}[variant]


def time_embedding(variant, sd, t, labels=None, dtype=torch.float32):
    """The row vector every time_mlp reads (reference :338-339; generation: + label_emb(y) when labels are given)."""
    from oracle import unet_oracle as U
    emb = U.pos_encoding(t.unsqueeze(-1).type(torch.float), U.TIME_EMB_DIM).to(dtype)
    if variant == "generation" and labels is not None:
        emb = emb + F.embedding(labels, sd["label_emb.weight"])
    return emb


def stage_input_plus_temb(sd, taps, emb, i, mlp=None):
    """`ups.i.in`: the input of decoder stage i plus relu(time_mlp(t)) of ups.i.time_mlp, broadcast over the pixels
    (reference :199; unet_oracle._time_mlp applies the ReLU itself and returns (B, C, 1, 1))."""
    from oracle import unet_oracle as U
    src = taps["bottle_neck"] if i == 0 else taps[f"up_convs.{i - 1}"]
    return src + U._time_mlp(sd, mlp or f"ups.{i}.time_mlp", emb)


def derived_taps(variant, sd, taps, emb):
    """References of the plan's tensors the oracle does not name, from oracle taps and the state_dict alone."""
    enc, skip = _names(variant)
    d = {}
    if enc is not None:
        src = taps["upsampled_lr_img"] if variant == "superres" else taps[enc]
        d["cond"] = F.conv2d(src, sd[skip + ".weight"], sd[skip + ".bias"], padding=1)
    d["conv_blocks.0.skip"] = F.conv2d(taps["x0"], sd[f"conv_blocks.0.{skip}.weight"], sd[f"conv_blocks.0.{skip}.bias"], padding=1)
    for i in range(3):
        Cc = UP[i]
        a = f"attention_blocks.{i}"
        d[f"ups.{i}.in"] = stage_input_plus_temb(sd, taps, emb, i)
        # the att-half of up_convs.i as its own convolution, WITHOUT bias: pack_upfuse_stage_images (conv_api.hip) packs it with
        # a null bias, plan_pack.hip's ah_b_off holds zeros, and up_convs.i.bias is folded into the composite's bias instead
        d[f"up_convs.{i}.att_half"] = F.conv2d(taps[a], sd[f"up_convs.{i}.weight"][:, Cc:], None, padding=1)
        d[f"cat.{i}"] = torch.cat([taps[f"ups.{i}"], taps[a]], dim=1)
        # the five-launch gate's intermediates (reference :101-103)
        g1 = F.conv2d(taps[f"gating_signals.{i}"], sd[a + ".w_g.0.weight"], sd[a + ".w_g.0.bias"])
        d[a + ".g1"] = g1
        d[a + ".relu"] = F.relu(g1 + F.conv2d(taps[f"conv_blocks.{2 - i}"], sd[a + ".w_x.0.weight"], sd[a + ".w_x.0.bias"], stride=2))
    return d


def _oracle_run(variant, sd, x, t, cond, mag, labels):
    from oracle import unet_oracle as U
    taps = {}
    with torch.no_grad():
        if variant == "superres":
            out = U.unet_forward(sd, x, t, cond, mag, taps=taps)
        elif variant == "sar":
            out = U.unet_forward_sar(sd, x, t, cond, taps=taps)
        elif variant == "generation":
            out = U.unet_forward_generation(sd, x, t, labels, taps=taps)
        else:
            raise ValueError(variant)
        taps.update(derived_taps(variant, sd, taps, time_embedding(variant, sd, t, labels, x.dtype)))
    taps[OUTPUT] = out
    return taps


def oracle_taps(variant, sd, inputs, dtype=torch.float32):
    """{name: reference}, the network output under OUTPUT.  `inputs` = (x, t, cond, mag) with cond the LR / SAR image, or for
    the generation variant the labels (None: unconditional; -1 marks a row that runs unconditionally: eval forwards are
    independent per image, so those rows come from a second, unconditional forward).  dtype float64: the whole oracle in
    float64 (positional encoding in fp32 like the reference, see unet_oracle.pos_encoding)."""
    x, t, cond, mag = inputs
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.to(dtype)
    if variant != "generation":
        return _oracle_run(variant, sd, x, t, cond.to(dtype), mag, None)
    if cond is None or bool((cond >= 0).all()):
        return _oracle_run(variant, sd, x, t, None, 1, cond)
    lab = _oracle_run(variant, sd, x, t, None, 1, cond.clamp_min(0))
    unc = _oracle_run(variant, sd, x, t, None, 1, None)
    rows = (cond >= 0)[:, None, None, None]
    return {k: torch.where(rows, lab[k], unc[k]) for k in lab}


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------
FRAMES = (("all", (...,)), ("row0", (..., slice(0, 1), slice(None))), ("row-1", (..., slice(-1, None), slice(None))),
          ("col0", (..., slice(0, 1))), ("col-1", (..., slice(-1, None))))


def compare(live, want, tol):
    """Every tensor of `live` that has a reference in `want`, whole and on each of its four one-pixel border frames on the
    frame's own scale (borders are where patch and halo code goes wrong; an interior-dominated norm hides them), in both
    norms of conftest.rel_errors.  `tol`: one bar, or {(name, frame): bar} with the bar of "" for the entries not listed
    (frame: "all", "row0", "row-1", "col0", "col-1").
    Returns (table, worst) with rows (name, frame, max-rel, rel-L2, bar); prints the table, one line per tensor."""
    table = []
    for name in sorted(live):
        if name not in want:
            continue
        got, ref = live[name], want[name]
        assert tuple(got.shape) == tuple(ref.shape), f"{name}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
        for frame, sl in FRAMES:
            bar = tol.get((name, frame), tol[""]) if isinstance(tol, dict) else tol
            e_max, e_l2 = rel_errors(got[sl], ref[sl])
            table.append((name, frame, e_max, e_l2, bar))
    worst = max(table, key=lambda r: max(r[2], r[3]) / r[4])
    for name in sorted({r[0] for r in table}):
        rows = [r for r in table if r[0] == name]
        edge = max(rows[1:], key=lambda r: max(r[2], r[3]))
        print(f"  {name:28s} {tuple(live[name].shape)!s:20s} max-rel {rows[0][2]:.2e} rel-L2 {rows[0][3]:.2e}   worst frame "
              f"{edge[1]:5s} {edge[2]:.2e} / {edge[3]:.2e}   bar {rows[0][4]:.1e}")
    print(f"  worst: {worst[0]} [{worst[1]}] max-rel {worst[2]:.2e} rel-L2 {worst[3]:.2e}")
    return table, worst


def failures(table):
    """The rows of a `compare` table outside their bar (a NaN error counts as outside)."""
    return [r for r in table if not (r[2] <= r[4] and r[3] <= r[4])]


def assert_within(table, what=""):
    bad = sorted(failures(table), key=lambda r: -max(r[2], r[3]))
    assert not bad, f"{what}: " + ", ".join(f"{n}[{fr}] max-rel {a:.2e} rel-L2 {b:.2e} > {bar:.1e}" for n, fr, a, b, bar in bad[:10])


def check_ops(log, compared, written):
    """Every op of a launch log maps through OP_WRITES to a compared tensor or to the network output; the only ops that may map
    to nothing are those OP_WRITES gives no named result.  Every named tensor an op wrote is compared."""
    ops = sorted({op for op, _ in log if op})
    unknown = [op for op in ops if op not in OP_WRITES]
    assert not unknown, f"ops missing from taps.OP_WRITES: {unknown}"
    hollow, skipped = [], []
    for op in ops:
        names = OP_WRITES[op]
        if not names:
            continue
        if not any(n == OUTPUT or n in compared for n in names):
            hollow.append(op)
        skipped += [(op, n) for n in names if n in written and n not in compared]
    assert not hollow, f"ops none of whose results were compared: {hollow}"
    assert not skipped, f"written but not compared: {skipped}"
