"""GPU: pc_val_metrics (csrc/valmetrics.hip) against the float64 restatement of tests/test_valstep_cpu.py and against what the
reference's validate computed on tests/valfixture.py (tests/golden/val_epoch.npz).

Shapes: the smallest at which each part of the kernel can go wrong -- less than one wave (B 1, 2x2), one ragged block with a float4
tail (B 3, 5x7), several blocks per clip with a ragged last one (B 2, 56x56), the largest validation batch (B 16, 28x28) -- with 24
and 21 classes.  Counts and n_correct must be exact; each loss scalar may be no further from float64 than the larger of 1e-6 and twice
the distance of an fp32 torch evaluation of the same formulas on the CPU (the factor two allows for another summation order)."""
import numpy as np
import pytest
import torch

from picons_amd import ops, valstep
from tests.test_valstep_cpu import golden_batches, restate

pytestmark = pytest.mark.gpu
SHAPES = [(1, 2, 2), (3, 5, 7), (2, 56, 56), (16, 28, 28)]
LOSSES = ("total", "loc", "cls", "abs_cls", "bce", "dice")
_cases = {}


def make_case(B, H, W, C):
    """Random logits in +-10 with planted 0.0, -0.0, +-80, +-1e-7 (inside and outside the truth); one box per clip; where the batch has
    room, clip 0 has an empty truth (B >= 2) and the last clip no positive logit (B >= 3); row 0 of the scores ties its maximum at two
    classes with the action at the FIRST of them (correct), and (B >= 2) row 1 ties with the action at the SECOND (not correct)."""
    key = (B, H, W, C)
    if key in _cases:
        return _cases[key]
    g = np.random.default_rng(1000 * B + 10 * H + C)
    x = (20.0 * g.random((B, 1, 8, H, W)) - 10.0).astype(np.float32)
    y = np.zeros((B, 1, 8, H, W), np.float32)
    planted = np.array([0.0, -0.0, 80.0, -80.0, 1e-7, -1e-7], np.float32)
    for b in range(B):
        h, w = int(g.integers(1, H + 1)), int(g.integers(1, W + 1))
        y0, x0 = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
        y[b, 0, :, y0:y0 + h, x0:x0 + w] = 1.0
        if B >= 3 and b == B - 1:
            x[b] = -np.abs(x[b]) - 1e-3
        x[b, 0, 0:6, y0, x0] = planted                                  # inside the truth
        x[b, 0, 0:6, (y0 + h) % H, (x0 + w) % W] = planted[::-1]        # outside it, unless the box fills the frame
        if B >= 3 and b == B - 1:
            x[b] = np.minimum(x[b], np.float32(0.0) * np.sign(x[b]))    # keeps 0.0 / -0.0 / negatives, drops the planted positives
    if B >= 2:
        y[0] = 0.0
    p = g.random((B, C)).astype(np.float32)
    a = g.integers(0, C, B).astype(np.int32)
    p[0, 3] = p[0, 7] = 2.0
    a[0] = 3
    if B >= 2:
        p[1, 2] = p[1, 5] = 2.0
        a[1] = 5
    for b in range(2, B, 2):
        a[b] = int(p[b].argmax())
    case = dict(logits=x, truth=y, scores=p, action=a)
    case["f64"] = restate(x, y, p, a, torch.float64)
    case["f32"] = restate(x, y, p, a, torch.float32)
    _cases[key] = case
    return case


def run_kernel(case):
    dev = "cuda:0"
    rec = ops.val_metrics(torch.from_numpy(case["logits"]).to(dev), torch.from_numpy(case["truth"]).to(dev), torch.from_numpy(case["scores"]).to(dev),
                          torch.from_numpy(case["action"]).to(dev))
    return rec


@pytest.mark.parametrize("C", [24, 21])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_val_metrics_vs_float64(B, H, W, C):
    """The test prints |kernel - f64| and |fp32 torch - f64| for every scalar before it asserts.  No MI355X run has been recorded yet
    (docs/EVAL_AND_INPUT.md 3c); on the CPU the fp32 torch evaluation sits 3e-9 .. 6e-7 from float64 on these cases."""
    case = make_case(B, H, W, C)
    rec = run_kernel(case)
    rec2 = run_kernel(case)
    assert torch.equal(rec, rec2)                                        # no atomics on floating-point data: bit-identical from run to run
    got, ref, f32 = ops.decode_val_record(rec), case["f64"], case["f32"]
    assert got["B"] == B and np.array_equal(got["counts"], ref["counts"]) and got["n_correct"] == ref["n_correct"]
    valid = [c for c in ref["counts"].tolist() if c[2] > 0]
    if B >= 2:
        assert len(valid) == B - 1                                        # the clip with gt = 0 is left out of the IoU mean
    assert got["iou_clips"] == len(valid)
    assert abs(got["iou_sum"] - sum(i / u for i, u, _g in valid)) <= 1e-6 * max(1, len(valid))
    s = valstep.summarize([got])
    assert s["validiou"] == len(valid) and s["total_IOU"] == sum(float(i) / float(u) for i, u, _g in valid)
    for k in LOSSES:
        d, d32 = abs(got[k] - ref[k]), abs(f32[k] - ref[k])
        print("val_metrics B=%d %dx%d C=%d %-7s f64 %.9g  |kernel-f64| %.3e  |fp32 torch-f64| %.3e" % (B, H, W, C, k, ref[k], d, d32))
    for k in LOSSES:
        assert abs(got[k] - ref[k]) <= max(2.0 * abs(f32[k] - ref[k]), 1e-6), k
    if B >= 2:
        assert ref["n_correct"] >= 1 and ref["n_correct"] < B              # the tie at the first maximum counts, the one at the second does not


def test_val_metrics_on_the_reference_golden(golden_dir):
    """The logits the reference's validate saw, through the kernel: its losses within 1e-4 (the project's bar for loss scalars), its
    accuracies and validiou exactly, its IoU sum within 1e-6."""
    g, gb = golden_batches(golden_dir)
    recs = []
    for k, b in enumerate(gb):
        r = ops.decode_val_record(run_kernel(dict(b, action=b["action"].astype(np.int32), truth=b["truth"].reshape(b["logits"].shape))))
        recs.append(r)
        print("golden batch %d: total %.7f (ref %.7f) loc %.7f (%.7f) cls %.7f (%.7f)" % (k, r["total"], g["total_loss"][k], r["loc"], g["loc_loss"][k],
                                                                                      r["cls"], g["class_loss"][k]))
        assert abs(r["total"] - g["total_loss"][k]) <= 1e-4 and abs(r["loc"] - g["loc_loss"][k]) <= 1e-4 and abs(r["cls"] - g["class_loss"][k]) <= 1e-4
        assert r["n_correct"] / r["B"] == g["accuracy"][k]
    s = valstep.summarize(recs, int(g["epoch"]))
    assert s["validiou"] == int(g["validiou"]) and abs(s["total_IOU"] - float(g["total_IOU"])) <= 1e-6
    assert abs(s["total"] - float(g["ret"])) <= 1e-4 and s["line"] == str(g["line"])


def test_out_of_range_action_poisons_the_class_losses_only():
    case = dict(make_case(3, 5, 7, 24))
    case["action"] = case["action"].copy()
    case["action"][1] = 24
    got = ops.decode_val_record(run_kernel(case))
    assert np.isnan(got["cls"]) and np.isnan(got["abs_cls"]) and np.isnan(got["total"])
    assert abs(got["loc"] - case["f64"]["loc"]) <= 1e-5 and np.array_equal(got["counts"], case["f64"]["counts"])
