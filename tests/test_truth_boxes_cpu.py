"""CPU: truth given as boxes, what is decided on the host, without a GPU.  evalstep.BoxTruth against the bbox arrays the reference's own
evaluation loader painted (tests/golden/eval_boxes.npz, tools/make_eval_boxes_golden.py) and against numpy slicing; flags against the dense
map inside the crop; the synthetic box videos against the dense ones; check_truth; the validation; the refusals of pc_paint_boxes before any
HIP call -- through capi, and as a stand-alone program under ASan + UBSan --; the constants and the Makefile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from picons_amd import capi, evalstep, ops, synthetic
from picons_amd.evalstep import BoxTruth

from tests import truth_boxes_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_boxes.npz")
vp = C.c_void_p
ORDER = ("rects", "R", "F", "H", "W", "f0", "nf", "binary", "truth")
OK = dict(rects=vp(64), R=3, F=4, H=5, W=7, f0=0, nf=4, binary=0, truth=vp(1027))
# (argument, value, a word of the message)
BAD = [("rects", None, b"null"), ("truth", None, b"null"),
       ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"), ("H", -1, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"),
       ("R", 0, b"R ="), ("R", -1, b"R ="), ("R", 33, b"R ="), ("R", 2 ** 31 - 1, b"R ="),
       ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
       ("rects", vp(65), b"rects must be"), ("rects", vp(66), b"rects must be"), ("rects", vp(67), b"rects must be")]
SIZE_BAD = [(1 << 16, 1 << 15), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2), (46341, 46341)]          # H * W >= 2^31


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _golden_cases():
    g = np.load(GOLDEN)
    for k in range(int(g["n"])):
        F, H, W = (int(v) for v in g["shape_%d" % k])
        anns = [(int(s), int(e), int(lab), g["boxes_%d_%d" % (k, i)].tolist(), g["annot_%d_%d" % (k, i)].tolist())
                for i, (s, e, lab) in enumerate(g["ann_%d" % k])]
        yield k, F, H, W, anns, int(g["seed_%d" % k]), g["bbox_%d" % k], int(g["label_%d" % k])


# ---------------------------------------------------------------------- against the reference's loader
def test_from_annotation_paints_what_the_reference_loader_painted():
    picks, n_anns = {}, {}
    for k, F, H, W, anns, seed, bbox, label in _golden_cases():
        assert F <= 12 and bbox.shape == (F, H, W) and bbox.dtype == np.uint8
        np.random.seed(seed)
        i = evalstep.pick_annotation(anns)
        picks.setdefault(len(anns), set()).add(i)
        n_anns[k] = len(anns)
        bt = BoxTruth.from_annotation(anns[i], F, H, W)
        assert bt.shape == (F, H, W) and bt.rects.shape == (F, 1, 5) and bt.rects.dtype == np.int32
        assert np.array_equal(bt.dense(), bbox), k                   # byte for byte
        assert np.array_equal(bt.dense(binary=True), bbox) and np.array_equal(ref.paint(bt.rects, F, H, W), bbox)
        assert anns[i][2] == label
    assert len(n_anns) >= 10 and set(picks) == {1, 2, 3}
    assert len(picks[2]) == 2 and len(picks[3]) >= 2                 # the draw mattered: the seeds pick different annotations


def test_pick_annotation_consumes_a_draw_only_with_more_than_one():
    np.random.seed(5)
    want = np.random.randint(0, 1 << 30)
    np.random.seed(5)
    assert evalstep.pick_annotation([("a",)]) == 0
    assert np.random.randint(0, 1 << 30) == want                     # nothing was drawn
    np.random.seed(5)
    first = np.random.randint(0, 3)
    np.random.seed(5)
    assert evalstep.pick_annotation([1, 2, 3]) == first


# ---------------------------------------------------------------------- clipping
def test_from_xywh_clips_as_numpy_slices():
    W = 5
    for x in range(-W - 2, W + 3):
        for w in range(0, W + 3):
            want = np.zeros((1, W, W), np.uint8)
            want[0, :, x:x + w] = 1
            bt = BoxTruth.from_xywh(np.array([[[x, 0, w, W]]]), W, W)
            assert np.array_equal(bt.dense(), want), (x, w)
            x0, x1, _ = slice(x, x + w).indices(W)
            assert bt.rects[0, 0, :2].tolist() == [x0, max(x1, x0)], (x, w)
            want = np.zeros((1, W, 3), np.uint8)                     # the same on the other axis
            want[0, x:x + w, :] = 1
            assert np.array_equal(BoxTruth.from_xywh(np.array([[[0, x, 3, w]]]), W, 3).dense(), want), (x, w)


def test_from_annotations_later_wins_and_values_are_the_actors():
    a = (0, 5, 2, [[2, 2, 8, 8]] * 6, [0])
    b = (2, 9, 2, [[6, 6, 8, 8]] * 8, [3])
    bt = BoxTruth.from_annotations([a, b], 8, 16, 20)
    assert bt.rects.shape == (8, 2, 5)
    d = bt.dense()
    want = np.zeros((8, 16, 20), np.uint8)
    want[0:6, 2:10, 2:10] = 1
    want[2:8, 6:14, 6:14] = 2
    assert np.array_equal(d, want)
    assert d[3, 7, 7] == 2 and d[3, 3, 3] == 1 and d[0, 7, 7] == 1 and d[7, 7, 7] == 2 and d[6, 3, 3] == 0
    assert np.array_equal(bt.dense(binary=True), (want != 0).astype(np.uint8))
    assert np.array_equal(ref.paint(bt.rects, 8, 16, 20), want)
    one = BoxTruth.from_annotation(b, 8, 16, 20, value=7)
    assert set(np.unique(one.dense())) == {0, 7} and one.nbytes == 8 * 1 * 5 * 4
    assert not BoxTruth.from_annotations([], 3, 4, 4).dense().any()


# ---------------------------------------------------------------------- flags and clips
def _random_table(rng, F, R, H, W):
    r = np.zeros((F, R, 5), np.int64)
    x = np.sort(rng.integers(0, W + 1, (F, R, 2)), axis=2)
    y = np.sort(rng.integers(0, H + 1, (F, R, 2)), axis=2)
    r[..., 0:2], r[..., 2:4] = x, y
    r[..., 4] = rng.integers(0, 4, (F, R)) * rng.integers(0, 2, (F, R))
    r[rng.random((F, R)) < 0.5] = 0                                  # many empty slots, and frames without truth
    return r


def test_flags_are_the_dense_map_inside_the_crop_and_give_the_same_clips():
    rng = np.random.default_rng(7)
    some, none = 0, 0
    for trial in range(40):
        F, R, H, W = int(rng.integers(1, 40)), int(rng.integers(1, 4)), 30, 36
        S = int(rng.integers(4, 20))
        h0, w0 = int(rng.integers(0, H - S + 1)), int(rng.integers(0, W - S + 1))
        bt = BoxTruth((F, H, W), _random_table(rng, F, R, H, W))
        counts = (bt.dense()[:, h0:h0 + S, w0:w0 + S] != 0).reshape(F, -1).sum(axis=1)     # what pc_truth_frame_flags counts
        fl = bt.flags(h0, w0, S)
        assert fl.dtype == np.int32 and fl.shape == (F,) and np.array_equal(fl != 0, counts != 0), trial
        assert evalstep.clip_starts(F, fl, 2) == evalstep.clip_starts(F, counts, 2)
        some += int((fl != 0).sum())
        none += int((fl == 0).sum())
    assert some > 50 and none > 50


def test_synthetic_box_videos_are_the_dense_ones():
    for kw in (dict(), dict(hw=112, frames_hw=(120, 136))):
        dense = synthetic.make_eval_videos_u8(4, **kw)
        boxes = synthetic.make_eval_videos_boxes(4, **kw)
        assert len(boxes) == 4
        for (fa, ta, la), (fb, tb, lb) in zip(dense, boxes):
            assert isinstance(tb, BoxTruth) and np.array_equal(fa, fb) and la == lb
            assert tb.shape == ta.shape[:3] and np.array_equal(tb.dense(binary=True), ta[..., 0])
            assert tb.nbytes < ta.nbytes // 100
        hw = kw.get("hw", 224)
        H, W = boxes[1][1].shape[1:]
        h0, w0 = evalstep.centre_crop(H, W, hw)
        assert not boxes[1][1].flags(h0, w0, hw).any() and boxes[1][1].dense().any()          # video 1: truth, none of it inside the crop
        assert boxes[0][1].flags(h0, w0, hw).any()


# ---------------------------------------------------------------------- check_truth and the validation
def test_check_truth_takes_a_box_truth_of_the_right_shape():
    bt = BoxTruth((3, 8, 9), np.zeros((3, 2, 5), np.int32))
    assert evalstep.check_truth("score", bt, 3, 8, 9) is bt
    assert evalstep.check_truth("score", bt, 3, 8, 9, video=2) is bt
    for shape in ((4, 8, 9), (3, 9, 8), (3, 8, 10)):
        with pytest.raises(ValueError, match=r"score: truth of video 1 has shape \(3, 8, 9\), expected"):
            evalstep.check_truth("score", bt, *shape, video=1)
    with pytest.raises(ValueError, match=r"add_video: truth has shape"):
        evalstep.check_truth("add_video", bt, 3, 8, 8)
    bt.rects = np.zeros((3, 33, 5), np.int32)                        # a table swapped behind the constructor's back
    with pytest.raises(ValueError, match="R in 1..32"):
        evalstep.check_truth("score", bt, 3, 8, 9)
    # a dense truth is treated as it was
    t = np.zeros((3, 8, 9, 1), np.uint8)
    assert tuple(evalstep.check_truth("score", t, 3, 8, 9).shape) == (3, 8, 9)
    with pytest.raises(ValueError, match="has shape"):
        evalstep.check_truth("score", t, 3, 8, 8)


def test_every_validation_failure_is_a_value_error():
    ok = np.array([[[1, 4, 2, 6, 9]]])
    assert BoxTruth((1, 8, 9), ok).rects.tolist() == ok.tolist()
    BoxTruth((1, 8, 9), np.array([[[0, 9, 0, 8, 255]]]))             # the whole frame, the largest value
    BoxTruth((1, 8, 9), np.array([[[4, 4, 8, 8, 0]]]))               # empty at the far edge
    bad = [np.array([[[-1, 4, 2, 6, 1]]]), np.array([[[5, 4, 2, 6, 1]]]), np.array([[[1, 10, 2, 6, 1]]]),        # x
           np.array([[[1, 4, -1, 6, 1]]]), np.array([[[1, 4, 7, 6, 1]]]), np.array([[[1, 4, 2, 9, 1]]]),         # y
           np.array([[[1, 4, 2, 6, -1]]]), np.array([[[1, 4, 2, 6, 256]]]),                                      # value
           np.zeros((1, 0, 5), np.int32), np.zeros((1, 33, 5), np.int32),                                        # R
           np.zeros((2, 1, 5), np.int32), np.zeros((1, 1, 4), np.int32), np.zeros((1, 5), np.int32), np.zeros((1, 1, 5), np.float32)]
    for r in bad:
        with pytest.raises(ValueError, match="BoxTruth"):
            BoxTruth((1, 8, 9), r)
    for shape in ((0, 8, 9), (1, 0, 9), (1, 8, 0), (1, 8), "abc"):
        with pytest.raises(ValueError, match="BoxTruth"):
            BoxTruth(shape, np.zeros((1, 1, 5), np.int32))
    for boxes, values in ((np.zeros((1, 1, 5), np.int64), None), (np.zeros((1, 2, 4), np.float32), None), (np.zeros((1, 2, 4), np.int64), [1]),
                          (np.zeros((1, 2, 4), np.int64), [1, 256]), (np.zeros((1, 33, 4), np.int64), None)):
        with pytest.raises(ValueError, match="BoxTruth"):
            BoxTruth.from_xywh(boxes, 8, 9, values)
    with pytest.raises(ValueError, match="BoxTruth"):
        BoxTruth.from_annotation((-1, 3, 0, [[0, 0, 1, 1]] * 5, []), 4, 8, 9)


# ---------------------------------------------------------------------- the entry
def _refused(lib, args, word):
    rc = lib.pc_paint_boxes(*[args[k] for k in ORDER], None)
    assert rc == -1, (args, rc)                              # PC_E_ARG, before any HIP call (there is no device here to make one on)
    msg = lib.pc_last_error()
    assert word in msg and b"pc_paint_boxes" in msg, (word, msg)


def test_paint_boxes_refuses_bad_arguments_without_gpu(built):
    for key, val, word in BAD:
        _refused(built, dict(OK, **{key: val}), word)
    for H, W in SIZE_BAD:
        _refused(built, dict(OK, H=H, W=W), b"2^31")
    _refused(built, dict(OK, F=2 ** 31 - 1, f0=2 ** 31 - 1, nf=2 ** 31 - 1), b"f0")          # f0 + nf beyond int32


def test_ops_paint_boxes_refuses_cpu_tensors_and_bad_operands():
    r = torch.zeros(4, 2, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.paint_boxes(r, 4, 8, 9)
    for bad, F in ((torch.zeros(4, 2, 5), 4), (torch.zeros(4, 2, 5, dtype=torch.int32)[:, :, ::2], 4), (torch.zeros(4, 10, dtype=torch.int32), 4),
                   (np.zeros((4, 2, 5), np.int32), 4)):
        with pytest.raises(ValueError, match="paint_boxes"):
            ops.paint_boxes(bad, F, 8, 9)
    for shape in ((0, 8, 9), (4, 0, 9), (4, 8, 0), (4, 1 << 16, 1 << 15)):
        with pytest.raises(ValueError, match="paint_boxes"):
            ops.paint_boxes(r, *shape)


def test_host_side_of_the_entry_under_asan_ubsan():
    """Every refusal path as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded into Python):
    tests/truth_boxes_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/truth_boxes_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "truth_boxes_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    assert "pc_paint_boxes" in capi.EXPORTS and re.search(r"\bpc_paint_boxes\(", header)
    getattr(built, "pc_paint_boxes")
    assert int(re.search(r"#define\s+PC_BOX_MAX\s+(\d+)", header).group(1)) == ops.BOX_MAX == BoxTruth.MAX_RECTS == ref.MAX_RECTS == 32
    assert int(re.search(r"#define\s+PC_BOX_WORDS\s+(\d+)", header).group(1)) == ops.BOX_WORDS == BoxTruth.WORDS == ref.WORDS == 5
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\btruth_boxes\b", mk, re.M) and re.search(r"^SRCS\s*=.*\btruthboxes\.hip\b", mk, re.M)
