"""CPU: what scoring a detection pass against truth decides on the host, without a GPU.  The numpy restatement of pc_map_crosstab
(tests/map_crosstab_ref.py) on a case counted by hand; detect.crosstab_counts against the definition of pc_seg_frame_counts;
detect.accumulate_video against the reference's loop as oracle.evalmetrics restates it, ties on a threshold included;
detect.instance_actor_iou; the refusals of pc_map_crosstab before any HIP call -- through capi, and as a stand-alone program under ASan +
UBSan --, pc_map_crosstab_ws_bytes, and the names and constructors the feature must not touch."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle import evalmetrics as oeval
from picons_amd import capi, detect, evalmetrics, evalstep, ops

from tests import map_crosstab_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
ORDER = ("pred", "truth", "F", "H", "W", "f0", "nf", "P", "A", "out", "ws")
OK = dict(pred=vp(65), truth=vp(1027), F=4, H=12, W=12, f0=0, nf=4, P=1, A=1, out=vp(2048), ws=vp(4096))
# (argument, value, a word of the message)
BAD = [("pred", None, b"null"), ("truth", None, b"null"), ("out", None, b"null"), ("ws", None, b"null"),
       ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"), ("H", -1, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"),
       ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
       ("P", 0, b"P ="), ("P", -1, b"P ="), ("P", 33, b"P ="), ("P", 2 ** 31 - 1, b"P ="), ("A", 0, b"A ="), ("A", -5, b"A ="), ("A", 33, b"A ="),
       ("A", 255, b"A ="), ("out", vp(2049), b"out must be"), ("out", vp(2050), b"out must be"), ("out", vp(2051), b"out must be"),
       ("ws", vp(4097), b"ws must be"), ("ws", vp(4098), b"ws must be"), ("ws", vp(4100), b"ws must be"), ("ws", vp(4103), b"ws must be")]
SIZE_BAD = [(1 << 16, 1 << 15), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2), (46341, 46341)]          # H * W >= 2^31


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _refused(lib, args, word):
    rc = lib.pc_map_crosstab(*[args[k] for k in ORDER], None)
    assert rc == -1, (args, rc)                              # PC_E_ARG, before any HIP call (there is no device here to make one on)
    msg = lib.pc_last_error()
    assert word in msg and b"pc_map_crosstab" in msg, (word, msg)


# ---------------------------------------------------------------------- the entries
def test_map_crosstab_refuses_bad_arguments_without_gpu(built):
    for key, val, word in BAD:
        _refused(built, dict(OK, **{key: val}), word)
    for H, W in SIZE_BAD:
        _refused(built, dict(OK, H=H, W=W), b"2^31")
    _refused(built, dict(OK, F=2 ** 31 - 1, f0=2 ** 31 - 1, nf=2 ** 31 - 1), b"f0")          # f0 + nf beyond int32


def test_ws_bytes_is_host_arithmetic_and_minus_one_where_the_call_refuses(built):
    ws = built.pc_map_crosstab_ws_bytes
    assert ws(1, 1, 1, 1, 1) == 9 * 4                        # one block, a 3 x 3 table
    assert ws(3, 5, 7, 8, 3) == 3 * 10 * 5 * 4
    assert ws(40, 240, 320, 1, 1) == 40 * 19 * 9 * 4         # 19200 groups of four at 1024 a block
    assert ws(1, 1080, 1920, 32, 32) == 64 * 34 * 34 * 4     # the cap of 64 blocks per frame at the largest table
    assert ws(1, 1, 256 * 1024, 1, 1) == 64 * 9 * 4 and ws(1, 1, 63 * 4096, 1, 1) == 63 * 9 * 4
    assert ws(2 ** 31 - 1, 46340, 46340, 32, 32) == (2 ** 31 - 1) * 64 * 1156 * 4          # the largest of all: no overflow in int64
    assert ops.map_crosstab_ws_bytes(40, 240, 320, 1, 1) == ws(40, 240, 320, 1, 1)
    for bad in ((0, 4, 4, 1, 1), (-1, 4, 4, 1, 1), (1, 0, 4, 1, 1), (1, 4, 0, 1, 1), (1, -4, -4, 1, 1), (1, 1 << 16, 1 << 15, 1, 1),
                (1, 2 ** 31 - 1, 2 ** 31 - 1, 1, 1), (1, 4, 4, 0, 1), (1, 4, 4, 33, 1), (1, 4, 4, 1, 0), (1, 4, 4, 1, 33), (1, 4, 4, -2 ** 31, 1)):
        assert ws(*bad) == -1, bad
        with pytest.raises(ValueError):
            ops.map_crosstab_ws_bytes(*bad)


def test_host_side_of_the_entries_under_asan_ubsan():
    """Every refusal path and the workspace arithmetic as a stand-alone program against the sanitizer build of the library (no GPU, nothing
    loaded into Python): tests/map_crosstab_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/map_crosstab_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "map_crosstab_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_map_crosstab", "pc_map_crosstab_ws_bytes"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header)
        getattr(built, name)
    assert int(re.search(r"#define\s+PC_CROSS_MAX_SLOTS\s+(\d+)", header).group(1)) == ops.CROSS_MAX_SLOTS == 32
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\bmap_crosstab\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bcrosstab\.hip\b", mk, re.M)


def test_constructors_keep_their_last_parameters_and_score_is_a_method():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"
    assert list(inspect.signature(detect.DetectEngine.score).parameters) == ["self", "truths", "labels", "actors", "which", "videos"]
    sig = inspect.signature(detect.DetectEngine.score).parameters
    assert sig["actors"].default == 1 and sig["which"].default == "masks" and sig["videos"].default is None


# ---------------------------------------------------------------------- the table
HAND_PRED = [[0, 0, 1, 1, 2, 2, 255, 255], [0, 1, 2, 255, 0, 1, 2, 255]]
HAND_TRUTH = [[0, 1, 0, 1, 3, 200, 0, 3], [0, 0, 1, 1, 200, 3, 1, 3]]
# P = 2, A = 2: pred slots 0, 1, 2 and 3 (the 255); truth slots 0, 1 and 3 (3 and 200 lie above A; no pixel has truth 2: column 2 is empty)
HAND_TABLE = [[2, 1, 0, 1],        # predicted background: on truth background twice, on truth 1 once, on truth 200 once
              [2, 1, 0, 1],        # pred 1
              [0, 2, 0, 2],        # pred 2
              [1, 1, 0, 2]]        # pred 255


def test_the_case_counted_by_hand():
    pred, truth = np.array([HAND_PRED], np.uint8), np.array([HAND_TRUTH], np.uint8)
    assert ref.slots([0, 1, 2, 3, 200, 255], 2).tolist() == [0, 1, 2, 3, 3, 3]
    t = ref.crosstab(pred, truth, 2, 2)
    assert t.dtype == np.int32 and t.shape == (1, 4, 4) and t[0].tolist() == HAND_TABLE and int(t.sum()) == 16
    assert detect.crosstab_counts(t).tolist() == [[9, 14, 11]]            # foreground on both sides, on either, in the truth
    assert detect.crosstab_counts(t).dtype == np.int64
    # the same pixels at P = 1, A = 1: everything non-zero is one slot or the other
    t1 = ref.crosstab(pred, truth, 1, 1)
    assert t1[0].tolist() == [[2, 1, 1], [2, 1, 1], [1, 3, 4]] and detect.crosstab_counts(t1).tolist() == [[9, 14, 11]]
    assert np.array_equal(ops.decode_map_crosstab(t.reshape(-1), 2, 2), t) and ops.decode_map_crosstab(t.reshape(-1), 2, 2).dtype == np.int32
    iou = detect.instance_actor_iou(t)
    assert iou.shape == (1, 2, 2) and iou.dtype == np.float64
    # rank 0 (pred 1: 4 pixels) with actor 1 (truth 1: 5 pixels) shares 1; rank 1 (pred 2: 4 pixels) shares 2; actor 2 has no pixel
    assert iou[0].tolist() == [[1 / 8, 0.0], [2 / 7, 0.0]]


def test_crosstab_counts_are_the_seg_frame_counts_of_a_binary_truth():
    rng = np.random.default_rng(20261020)
    for shape, dp, dt in (((5, 9, 13), 0.3, 0.4), ((3, 1, 1), 0.5, 0.5), ((4, 7, 5), 0.0, 0.6), ((4, 7, 5), 0.7, 0.0), ((2, 6, 6), 1.0, 1.0)):
        pred = (rng.random(shape) < dp).astype(np.uint8)
        truth = (rng.random(shape) < dt).astype(np.uint8)
        t = ref.crosstab(pred, truth, 1, 1)
        assert np.array_equal(t.reshape(shape[0], -1).sum(1), np.full(shape[0], shape[1] * shape[2]))
        assert np.array_equal(detect.crosstab_counts(t), ref.seg_counts(pred, truth))
        # more slots split the foreground, the triple stays
        ranks = (pred * rng.integers(1, 12, shape)).astype(np.uint8)
        assert np.array_equal(detect.crosstab_counts(ref.crosstab(ranks, truth, 8, 3)), ref.seg_counts(pred, truth))
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 1, 3), np.int32)):
        with pytest.raises(ValueError):
            detect.crosstab_counts(bad)


def test_instance_actor_iou_with_an_empty_cell():
    t = np.zeros((2, 4, 5), np.int32)                        # P = 2, A = 3
    t[0, 1, 1], t[0, 1, 0], t[0, 0, 1], t[0, 3, 1] = 6, 2, 3, 1          # rank 0: 8 pixels; actor 1: 10 pixels; 6 shared
    t[0, 2, 4] = 5                                           # rank 1 lies on "other" truth only
    iou = detect.instance_actor_iou(t)
    assert iou.shape == (2, 2, 3)
    assert iou[0, 0, 0] == 6 / (8 + 10 - 6) and iou[0, 1, 0] == 0.0 and iou[0, 0, 1] == 0.0
    assert iou[0, 1, 1] == 0.0 and iou[0, 1, 2] == 0.0       # actor 2, actor 3: no pixel; rank 1 has 5: inter 0 over 5
    assert not np.isnan(iou).any() and (iou[1] == 0.0).all()  # frame 1: every denominator is 0
    with pytest.raises(ValueError):
        detect.instance_actor_iou(np.zeros((2, 2, 3), np.int32))


# ---------------------------------------------------------------------- the evaluator's tables
N_PIX = 40


def _oracle_add(st, counts, label, fin_pred):
    """One video into the oracle's accumulators: frames of N_PIX pixels laid out so that the reference's own loop counts (inter, union, gt)."""
    counts = np.asarray(counts)
    F = counts.shape[0]
    n = -(-F // 8)
    logits, gt = np.full((n * 8, N_PIX), -4.0, np.float32), np.zeros((n * 8, N_PIX), np.int64)
    for f, (i, u, g) in enumerate(counts.tolist()):
        assert 0 <= i <= g <= u <= N_PIX
        gt[f, :g] = 1
        logits[f, :i] = 4.0                                  # predicted on truth
        logits[f, g:u] = 4.0                                 # predicted off truth
    pred = np.zeros((n, st.n_classes), np.float32)
    pred[:, fin_pred] = 1.0
    st.add_video(logits.reshape(n, 1, 8, 1, N_PIX), gt.reshape(n * 8, 1, N_PIX, 1), pred, label)


def _random_counts(rng, F):
    u = rng.integers(1, N_PIX + 1, F)
    g = np.array([rng.integers(0, x + 1) for x in u])
    g[0] = max(g[0], 1)                                      # a video passed to the accumulation holds truth somewhere
    i = np.array([rng.integers(0, x + 1) for x in g])
    return np.stack([i, u, g], axis=1).astype(np.int64)


def test_accumulate_video_is_the_reference_loop():
    rng = np.random.default_rng(7)
    C_ = 5
    videos = [(_random_counts(rng, F), int(rng.integers(0, C_))) for F in (1, 8, 17, 40)]
    # ratios exactly on a threshold: 1/4 and 1/2 are float32 numbers and hit their k; 3/20 lies BELOW float32(3) / 20 = 0.15000000596
    videos.append((np.array([[1, 4, 2], [2, 4, 3], [3, 20, 5], [10, 20, 10], [0, 7, 3]], np.int64), 2))
    # a frame without truth but with predicted pixels: it must not reach the video's sums (with it the video's ratio falls below 1/2)
    videos.append((np.array([[4, 8, 4], [0, 30, 0], [0, 0, 0]], np.int64), 3))
    videos.append((np.array([[3, 20, 20]], np.int64), 4))                   # the video's own ratio on the 3/20 tie
    acc, st = evalmetrics.MapAccumulator(C_, device="cpu"), oeval.MapState(C_)
    for counts, label in videos:
        detect.accumulate_video(counts, label, acc)
        _oracle_add(st, counts, label, label)
    got = acc.result()
    assert np.array_equal(got["frame_ious"], st.frame_ious) and np.array_equal(got["video_ious"], st.video_ious)
    assert np.array_equal(got["n_tot_frames"], st.n_tot_frames) and np.array_equal(got["n_vids"], st.n_vids)
    want = st.result()
    for k in ("fmAP", "vmAP"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    # the ties, spelled out
    one = evalmetrics.MapAccumulator(C_, device="cpu")
    detect.accumulate_video(np.array([[1, 4, 2]]), 0, one)
    assert one.frame_hits[0].tolist() == [1] * 6 + [0] * 14                 # 0.25 >= k / 20 up to k = 5
    detect.accumulate_video(np.array([[3, 20, 5]]), 1, one)
    assert one.frame_hits[1].tolist() == [1] * 3 + [0] * 17                 # 0.15 < float32(0.15): k = 3 is missed
    detect.accumulate_video(np.array([[10, 20, 10]]), 2, one)
    assert one.frame_hits[2].tolist() == [1] * 11 + [0] * 9 and one.video_hits[2].tolist() == [1] * 11 + [0] * 9
    detect.accumulate_video(np.array([[4, 8, 4], [0, 30, 0]]), 3, one)
    assert one.video_hits[3].tolist() == [1] * 11 + [0] * 9 and int(one.n_frames[3]) == 1 and int(one.n_vids[3]) == 1
    with pytest.raises(ValueError):
        detect.accumulate_video(np.array([[1, 4, 2]]), C_, one)


def test_score_pass_skips_a_video_without_truth_and_keeps_the_evaluators_keys():
    C_ = 4
    t_hit = np.zeros((2, 3, 3), np.int32)
    t_hit[:, 1, 1], t_hit[:, 0, 0] = 5, 11
    t_none = np.zeros((3, 3, 3), np.int32)                   # predicted pixels, no truth at all
    t_none[:, 1, 0], t_none[:, 0, 0] = 4, 12
    ps = detect.score_pass([t_hit, t_none, t_hit], [1, 2, 3], [1, 2, 0], C_)
    assert isinstance(ps, detect.PassScore) and [type(v) for v in ps.videos] == [detect.VideoScore] * 3
    assert set(ps.result) == set(evalmetrics.MapAccumulator(C_, device="cpu").result())
    assert set(ps.result) == {"accuracy", "fmAP", "vmAP", "frame_ious", "video_ious", "n_tot_frames", "n_vids", "n_correct"}
    assert ps.n_skipped == 1 and [v.skipped for v in ps.videos] == [False, True, False]
    assert [v.correct for v in ps.videos] == [True, False, False] and ps.result["n_correct"] == 1 and ps.result["accuracy"] == 0.5
    assert ps.result["n_vids"].reshape(-1).tolist() == [0, 1, 0, 1] and ps.result["n_tot_frames"].reshape(-1).tolist() == [0, 2, 0, 2]
    v0, v1 = ps.videos[0], ps.videos[1]
    assert v0.counts.tolist() == [[5, 5, 5]] * 2 and v0.frame_iou.tolist() == [1.0, 1.0] and v0.video_iou == 1.0
    assert (v0.label, v0.predicted, v1.label, v1.predicted) == (1, 1, 2, 2)
    assert np.isnan(v1.frame_iou).all() and np.isnan(v1.video_iou) and v1.counts.tolist() == [[0, 4, 0]] * 3
    assert v0.instance_iou().shape == (2, 1, 1) and v0.instance_iou()[0, 0, 0] == 1.0
    empty = detect.score_pass([], [], [], C_)
    assert empty.videos == [] and empty.n_skipped == 0 and empty.result["n_correct"] == 0


@pytest.mark.parametrize("who", ["score", "sweep"])
def test_truth_label_and_count_checks_refuse_what_score_and_sweep_refuse(who):
    """The bad truths / bad labels of tests/test_detect_score_gpu.py::test_refusals_are_value_errors_before_anything_is_enqueued against the
    pure functions both calls (and EvalEngine.add_video) check with: ValueError, `who` in front, the word the GPU test matches inside."""
    F, H, W, C_ = 3, 8, 12, 24
    every = [np.zeros((F, H, W), np.uint8) for _ in range(3)]
    for truths, labels, n, word in ((every, [0, 1, 2], 2, "truths"), (every[:2], [0, 1, 2], 3, "truths"), (every, [0, 1], 3, "labels")):
        with pytest.raises(ValueError, match="^%s: .*%s" % (who, word)):
            evalstep.check_counts(who, truths, labels, n)
    truths, labels = evalstep.check_counts(who, iter(every), (0, 1, 2), 3)
    assert isinstance(truths, list) and isinstance(labels, list) and labels == [0, 1, 2] and all(a is b for a, b in zip(truths, every))
    for label in (24, -1, 1.5, None, "one", 1 << 40):
        with pytest.raises(ValueError, match="^%s: label" % who):
            evalstep.check_label(who, label, C_)
    assert [evalstep.check_label(who, l, C_) for l in (0, 23, np.int64(5), 7.0)] == [0, 23, 5, 7]
    good = every[1]
    for bad, word in ((good[:2], "shape"), (good[:, :, :10], "shape"), (good[:, :6], "shape"), (good[..., None, None], "shape"), (good[0], "shape"),
                      (good.astype(np.float32), "uint8"), (good.astype(np.int32), "uint8"), (good.tolist(), "uint8"), (None, "uint8")):
        with pytest.raises(ValueError, match="^%s: truth of video 1.*%s" % (who, word)):
            evalstep.check_truth(who, bad, F, H, W, 1)
        with pytest.raises(ValueError, match="^%s: truth.*%s" % (who, word)):
            evalstep.check_truth(who, bad, F, H, W)
    for ok in (good, good[..., None], torch.from_numpy(good), torch.from_numpy(good)[..., None]):
        t = evalstep.check_truth(who, ok, F, H, W, 1)
        assert torch.is_tensor(t) and t.dtype == torch.uint8 and tuple(t.shape) == (F, H, W) and t.data_ptr() == torch.from_numpy(good).data_ptr()
