"""CPU: the validation pass without a GPU.  A float64 torch restatement of what pc_val_metrics computes (written here, used by the GPU
tests too) reproduces what the reference's own val_model_interface / validate computed on tests/valfixture.py
(tests/golden/val_epoch.npz, tools/make_val_golden.py); valstep.summarize turns records into validate's return value and printed line;
the C entry refuses bad arguments before any HIP call; the record / workspace sizes are the ones valstep lays its buffers out by."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from picons_amd import capi, ops, valstep
from tests import valfixture


def restate(logits, truth, scores, action, dtype=torch.float64):
    """One batch in torch on the CPU, in `dtype`: the formulas of val_model_interface (BCEWithLogits + Dice + SpreadLoss with margin 0.2 and
    the double division by b) and of validate's loop body (mask `logits > 0`, IOU2's sums, first-maximum arg-max).
    -> dict(total, loc, cls, abs_cls, bce, dice: Python floats; counts int64 [B][3] = inter, union, gt; n_correct)."""
    x = torch.as_tensor(np.asarray(logits)).to(dtype).reshape(len(logits), -1)
    y = torch.as_tensor(np.asarray(truth)).to(dtype).reshape(len(logits), -1)
    p = torch.as_tensor(np.asarray(scores)).to(dtype)
    a = torch.as_tensor(np.asarray(action)).long().reshape(-1)
    b = x.shape[0]
    bce = (torch.clamp(x, min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).mean()
    s = 1.0 / (1.0 + torch.exp(-x))
    dice = 1 - (2.0 * (s * y).sum() + 1) / (s.sum() + y.sum() + 1)
    at = p.gather(1, a.view(b, 1)).expand_as(p)
    cls = ((torch.clamp(0.2 - (at - p), min=0) ** 2).sum() / b - 0.2 ** 2) / b
    acls = (torch.clamp(0.9 - (at - p), min=0) ** 2).sum() / b - 0.9 ** 2
    on, t = x > 0, y != 0
    counts = torch.stack([(on & t).sum(1), (on | t).sum(1), t.sum(1)], 1).numpy().astype(np.int64)
    pn = p.numpy()
    best = np.array([int(np.flatnonzero(r == r.max())[0]) for r in pn])           # the first maximum, as torch.max on the CPU
    loc = bce + dice
    return dict(total=float(loc + cls), loc=float(loc), cls=float(cls), abs_cls=float(acls), bce=float(bce), dice=float(dice),
                counts=counts, n_correct=int((best == a.numpy()).sum()))


def golden_batches(golden_dir):
    g = np.load(os.path.join(golden_dir, "val_epoch.npz"))
    out, o = [], 0
    for n in g["sizes"].tolist():
        out.append(dict(logits=g["logits"][o:o + n], truth=g["truth"][o:o + n].astype(np.float32), scores=g["scores"][o:o + n], action=g["action"][o:o + n]))
        o += n
    return g, out


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def test_fixture_is_what_the_golden_recorded(golden_dir):
    """The stand-in network on the fixture's batches gives the logits / scores the golden holds, and the fixture has the cases it promises."""
    g, gb = golden_batches(golden_dir)
    net = valfixture.ValNet()
    for mb, ref in zip(valfixture.batches(), gb):
        with torch.no_grad():
            seg, pred, _ = net(torch.from_numpy(mb["data"]))
        assert np.array_equal(seg.numpy(), ref["logits"]) and np.allclose(pred.numpy(), ref["scores"], atol=1e-6)
        assert np.array_equal(mb["loc_msk"].astype(np.float32), ref["truth"]) and np.array_equal(mb["action"].reshape(-1), ref["action"])
    lg = g["logits"]
    assert ((lg == 0) & ~np.signbit(lg)).any() and ((lg == 0) & np.signbit(lg)).any() and (lg == 80).any() and (lg == -80).any()
    per_clip_truth = g["truth"].reshape(len(lg), -1).sum(1)
    assert (per_clip_truth == 0).sum() == 1                                             # one clip with an empty truth
    assert ((lg.reshape(len(lg), -1) > 0).sum(1)[per_clip_truth > 0] == 0).sum() == 1    # one clip with truth and no positive logit
    top2 = np.sort(g["scores"], axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 1e-4                                       # no arg-max ties


def test_float64_restatement_reproduces_the_reference(golden_dir):
    g, gb = golden_batches(golden_dir)
    iou_sum, valid = 0.0, 0
    for k, b in enumerate(gb):
        r = restate(**b)
        assert abs(r["total"] - g["total_loss"][k]) <= 1e-6 and abs(r["loc"] - g["loc_loss"][k]) <= 1e-6 and abs(r["cls"] - g["class_loss"][k]) <= 1e-6
        assert r["n_correct"] / len(b["action"]) == g["accuracy"][k]
        for inter, union, gt in r["counts"].tolist():
            if gt > 0:
                iou_sum += inter / union
                valid += 1
    assert valid == int(g["validiou"])
    assert abs(iou_sum - float(g["total_IOU"])) <= 1e-6          # the reference divides in float32


def test_summarize_gives_the_reference_return_value_and_line(golden_dir):
    g, gb = golden_batches(golden_dir)
    recs = []
    for k, b in enumerate(gb):
        n = len(b["action"])
        recs.append(dict(total=float(g["total_loss"][k]), loc=float(g["loc_loss"][k]), cls=float(g["class_loss"][k]),
                         n_correct=int(round(float(g["accuracy"][k]) * n)), B=n, counts=restate(**b)["counts"]))
    s = valstep.summarize(recs, int(g["epoch"]))
    assert abs(s["total"] - float(g["ret"])) <= 1e-6
    assert s["line"] == str(g["line"])
    assert s["validiou"] == int(g["validiou"]) and abs(s["total_IOU"] - float(g["total_IOU"])) <= 1e-6
    assert abs(s["accuracy"] - float(np.mean(g["accuracy"]))) <= 1e-12
    # a pass without a single clip with truth prints 0 instead of dividing by zero, as the drop-in's validate does
    empty = valstep.summarize([dict(total=1.0, loc=0.5, cls=0.5, n_correct=0, B=2, counts=np.zeros((2, 3), np.int32))], 1)
    assert empty["average_IOU"] == 0.0 and empty["line"].endswith("[IOU ] 0.000")
    with pytest.raises(ValueError):
        valstep.summarize([])


def test_bad_arguments_are_refused_without_gpu(built):
    ok = dict(output=C.c_void_p(64), loc_msk=C.c_void_p(128), pred=C.c_void_p(64), action=C.c_void_p(64), B=2, pix=32, C=24, record=C.c_void_p(64),
              ws=C.c_void_p(256))
    order = ("output", "loc_msk", "pred", "action", "B", "pix", "C", "record", "ws")
    bad = [(k, None, b"null") for k in ("output", "loc_msk", "pred", "action", "record", "ws")]
    bad += [("pix", 30, b"multiple of 4"), ("pix", 0, b"multiple of 4"), ("pix", -4, b"multiple of 4"), ("output", C.c_void_p(68), b"16-byte"),
            ("loc_msk", C.c_void_p(72), b"16-byte"), ("ws", C.c_void_p(264), b"16-byte"), ("B", 0, b"B = 0"), ("B", -1, b"B = -1"), ("C", 0, b"C = 0")]
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        rc = built.pc_val_metrics(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                       # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error(), (key, val, built.pc_last_error())


def test_host_side_of_pc_val_metrics_under_asan_ubsan():
    """The entry's argument checks and size arithmetic as a stand-alone program against the sanitizer build of the library (no GPU, nothing
    loaded into Python): tests/valmetrics_host_driver.cpp."""
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/valmetrics_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "valmetrics_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_sizes_agree_with_the_layout_valstep_assumes(built):
    for B in (1, 3, 16):
        assert ops.val_record_words(B) == ops.VAL_HEAD + 3 * B == 10 + 3 * B
    for B, pix in ((1, 32), (3, 280), (2, 25088), (16, 6272), (16, 8 * 224 * 224), (1, 4 * 1024 * 300)):
        nbx = min(max(-(-(pix // 4) // 1024), 1), 256)         # blocks per clip: ~4 float4 per thread, at most 256
        assert ops.val_metrics_ws_floats(B, pix) == 2 * (B * nbx * 4 + B * 4) + B * nbx * 4, (B, pix)
    assert ops.val_metrics_ws_floats(0, 32) == -1 and ops.val_metrics_ws_floats(2, 30) == -1 and ops.val_record_words(0) == -1
    # a record as the kernel writes it decodes to the names summarize reads
    rec = np.zeros(10 + 3 * 2, np.int32)
    rec[:8] = np.arange(1, 9, dtype=np.float32).view(np.int32)
    rec[8], rec[9] = 1, 2
    rec[10:] = [5, 9, 7, 0, 3, 0]
    d = ops.decode_val_record(rec)
    assert [d[k] for k in ops.VAL_SCALARS] == [1, 2, 3, 4, 5, 6, 7, 8] and d["n_correct"] == 1 and d["B"] == 2 and d["counts"].tolist() == [[5, 9, 7], [0, 3, 0]]
    assert valstep.summarize([d])["average_IOU"] == 5 / 9
    # the eval plan's metrics op: one record row of val_record_words(n) words, a workspace of at least the size the library asks for
    fake = SimpleNamespace(C=24, hw=72, per=8 * 72 * 72)
    p = valstep.ValEngine._plan(fake, 3)
    kind, i, _f, ptrs, l, lane = p.lists["fwd"][p.op_metrics]
    assert kind == capi.OP_VAL_METRICS and i == [3, 24] and l == [fake.per] and lane == 0 and p.op_metrics == len(p.lists["fwd"]) - 1
    assert ptrs[0] == p.out.ref and ptrs[1] == p.in_seg and ptrs[2] == p.pred and ptrs[3] == p.in_action and ptrs[4] is None
    assert p.arena_bytes - ptrs[5][1] >= 4 * ops.val_metrics_ws_floats(3, fake.per) and ptrs[5][1] % 16 == 0 and p.in_seg[1] % 16 == 0 and p.out.ref[1] % 16 == 0
    # begin() replays `prep` / `prep_late` once per pass: no op in them may read what a batch brings
    per_batch = {p.in_data, p.in_aug, p.in_cls, p.in_labeled, p.img.ref, p.in_seg, p.in_action}
    assert not any(r in per_batch for lst in ("prep", "prep_late") for op in p.lists[lst] for r in op[3] if r is not None)
