"""CPU self-test of tests/taps.py: `compare` passes an unmodified copy of the oracle's taps and flags each planted fault at
the 1e-4 bar of the default kernels' taps, and the written / untouched / partial classifier is right on NaN blocks."""
import pytest
import torch

import taps as T
from conftest import golden_inputs

TOL = 1e-4


@pytest.fixture(scope="module")
def base(seeded_sd):
    x, t, lr = golden_inputs("g3", 2, 2, 3, 16, 2, 1500)
    want = T.oracle_taps("superres", seeded_sd, (x, t, lr, 2))
    return want, (x, t, lr)


def _copy(want):
    return {k: v.clone() for k, v in want.items()}


def test_oracle_taps_hold_the_oracle_and_the_derived_references(base, golden, seeded_sd):
    want, (x, t, lr) = base
    for k, v in golden.items():  # the oracle's own taps are the reference's activations (G3)
        if k.startswith("g3_tap_"):
            assert torch.equal(want[k[len("g3_tap_"):]], torch.from_numpy(v)), k
    assert torch.equal(want[T.OUTPUT], torch.from_numpy(golden["g3_out"]))
    for i in range(3):
        Cc, Ch = T.UP[i], T.UP[i + 1]
        assert want[f"ups.{i}.in"].shape == (want["bottle_neck"] if i == 0 else want[f"up_convs.{i - 1}"]).shape
        assert want[f"up_convs.{i}.att_half"].shape == want[f"up_convs.{i}"].shape
        assert want[f"cat.{i}"].shape[1] == Cc + Ch
        # the two halves of up_convs.i add up to it: x-half + att-half (bias with the x-half, as the composite kernel has it)
        xh = torch.nn.functional.conv2d(want[f"ups.{i}"], seeded_sd[f"up_convs.{i}.weight"][:, :Cc],
                                        seeded_sd[f"up_convs.{i}.bias"], padding=1)
        assert torch.allclose(xh + want[f"up_convs.{i}.att_half"], want[f"up_convs.{i}"], rtol=1e-4, atol=1e-5)
        # ups.i.conv is the layer behind ups.i.in: conv + BatchNorm + ReLU of it reproduces the oracle's own tap
        from oracle import unet_oracle as U
        h = U._bn(seeded_sd, f"ups.{i}.batch_norm", U._conv(seeded_sd, f"ups.{i}.conv", want[f"ups.{i}.in"], padding=1), False, None)
        assert torch.equal(torch.relu(h), want[f"ups.{i}.conv"])


def test_unmodified_copy_passes(base):
    want, _ = base
    table, worst = T.compare(_copy(want), want, TOL)
    assert not T.failures(table)
    assert max(worst[2], worst[3]) == 0.0
    assert len({r[0] for r in table}) == len(want)


def test_scaled_border_row_of_one_channel_group_is_flagged(base):
    """Row 0 of channels 32 .. 63 of a 64-channel tensor scaled by 1 + 5e-4: what a wrong halo row of one patch's channel group
    looks like.  The frame's own norm sees it; every other tensor stays clean."""
    want, _ = base
    live = _copy(want)
    assert live["conv_blocks.1"].shape[1] == 64
    live["conv_blocks.1"][:, 32:64, 0, :] *= 1 + 5e-4
    bad = T.failures(T.compare(live, want, TOL)[0])
    assert {r[0] for r in bad} == {"conv_blocks.1"}
    assert "row0" in {r[1] for r in bad}
    with pytest.raises(AssertionError, match="conv_blocks.1"):
        T.assert_within(T.compare(live, want, TOL)[0], "planted")


def test_one_pixel_shift_is_flagged(base):
    want, _ = base
    for name in ("attention_blocks.2.psi", "up_convs.0.att_half", "x0"):
        live = _copy(want)
        live[name] = torch.roll(live[name], 1, dims=-1)
        bad = T.failures(T.compare(live, want, TOL)[0])
        assert {r[0] for r in bad} == {name}


def test_wrong_time_embedding_in_a_stage_input_is_flagged(base, seeded_sd):
    """`ups.1.in` built with stage 2's time embedding: conv_blocks.2.time_mlp, the other 128-row MLP of the network
    (ups.2.time_mlp has 64 rows and cannot be added to the 128 channels of this tensor at all)."""
    want, (x, t, lr) = base
    emb = T.time_embedding("superres", seeded_sd, t)
    live = _copy(want)
    live["ups.1.in"] = T.stage_input_plus_temb(seeded_sd, want, emb, 1, mlp="conv_blocks.2.time_mlp")
    bad = T.failures(T.compare(live, want, TOL)[0])
    assert {r[0] for r in bad} == {"ups.1.in"}
    # and the right one is the reference itself
    assert torch.equal(T.stage_input_plus_temb(seeded_sd, want, emb, 1), want["ups.1.in"])


def test_classifier_on_nan_blocks():
    nan = float("nan")
    clean = torch.arange(2 * 4 * 6 * 5, dtype=torch.float32).reshape(2, 4, 6, 5)
    assert T.classify(clean) == "written"
    assert T.classify(torch.full_like(clean, nan)) == "untouched"
    holed = clean.clone()
    holed[1, 1:3, 4:6, 2] = nan
    assert T.classify(holed) == "partial"
    assert T.nan_box(holed) == [(1, 1), (1, 2), (4, 5), (2, 2)]
    written, untouched = T.sort_tensors({"a": clean, "b": torch.full_like(clean, nan)})
    assert list(written) == ["a"] and untouched == ["b"]
    with pytest.raises(AssertionError, match=r"c \(2, 4, 6, 5\): NaN inside \[\(1, 1\), \(1, 2\), \(4, 5\), \(2, 2\)\]"):
        T.sort_tensors({"a": clean, "c": holed})
    # a concat buffer whose up-sampled slice never exists (composite stage) is judged through its slices: not live, no finding
    cat = torch.cat([torch.full((1, 64, 4, 4), nan), torch.ones(1, 32, 4, 4)], 1)
    written, untouched = T.sort_tensors({"cat.2": cat, "ups.2": cat[:, :64], "attention_blocks.2": cat[:, 64:]})
    assert list(written) == ["attention_blocks.2"] and untouched == ["cat.2", "ups.2"]
    written, _ = T.sort_tensors({"cat.2": torch.ones(1, 96, 4, 4), "ups.2": torch.ones(1, 64, 4, 4),
                                 "attention_blocks.2": torch.ones(1, 32, 4, 4)})
    assert sorted(written) == ["attention_blocks.2", "cat.2", "ups.2"]
    holed_slice = cat.clone()
    holed_slice[0, 70, 1, 1] = nan  # a hole inside a slice is still a finding, of the slice and of the buffer
    with pytest.raises(AssertionError, match="attention_blocks.2"):
        T.sort_tensors({"cat.2": holed_slice, "ups.2": holed_slice[:, :64], "attention_blocks.2": holed_slice[:, 64:]})


def test_check_ops_rejects_unknown_and_hollow_ops():
    log = [("conv0", "k"), ("", "gate_bias"), ("time_mlp", "k"), ("up_convs.2.fused", "k")]
    T.check_ops(log, {"x0"}, {"x0"})
    with pytest.raises(AssertionError, match="missing from taps.OP_WRITES"):
        T.check_ops(log + [("conv_blocks.0.new_fusion", "k")], {"x0"}, {"x0"})
    with pytest.raises(AssertionError, match="none of whose results were compared"):
        T.check_ops(log, set(), set())
    with pytest.raises(AssertionError, match="written but not compared"):
        T.check_ops(log + [("bottle_neck.conv2.0", "k")], {"x0", "ups.0.in"}, {"x0", "ups.0.in", "bottle_neck"})
