"""CPU: what sweeping the mask threshold of a detection pass decides on the host, without a GPU.  detect.threshold_words (0.5 is the word of
seg_positive); detect.sweep_counts against the definition -- the mask q >= word, threshold by threshold -- on maps that hold the words
themselves and their neighbours, and against crosstab_counts of the 0.5 mask; detect.sweep_pass at one threshold against score_pass on the
matching tables, bit for bit; SweepScore.best; the refusals of pc_prob_truth_hist before any HIP call -- through capi, and as a stand-alone
program under ASan + UBSan --, pc_prob_truth_hist_ws_bytes, and the names and constructors the feature must not touch."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, evalmetrics, ops

from tests import map_crosstab_ref as cref
from tests import prob_hist_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
ORDER = ("prob", "truth", "F", "H", "W", "f0", "nf", "thr", "N", "out", "ws")
THREE = (C.c_uint16 * 3)(100, 200, 300)                     # the words are HOST memory the entry reads: a real array, exactly N long
OK = dict(prob=vp(66), truth=vp(1027), F=4, H=12, W=12, f0=0, nf=4, thr=THREE, N=3, out=vp(2048), ws=vp(4096))
# (argument, value, a word of the message)
BAD = [("prob", None, b"null"), ("truth", None, b"null"), ("thr", None, b"null"), ("out", None, b"null"), ("ws", None, b"null"),
       ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"), ("H", -1, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"),
       ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
       ("N", 0, b"N ="), ("N", -1, b"N ="), ("N", 65, b"N ="), ("N", 2 ** 31 - 1, b"N ="), ("N", -2 ** 31, b"N ="),
       ("prob", vp(67), b"prob must be"), ("out", vp(2049), b"out must be"), ("out", vp(2050), b"out must be"), ("out", vp(2051), b"out must be"),
       ("ws", vp(4097), b"ws must be"), ("ws", vp(4098), b"ws must be"), ("ws", vp(4100), b"ws must be"), ("ws", vp(4103), b"ws must be")]
SIZE_BAD = [(1 << 16, 1 << 15), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2), (46341, 46341)]          # H * W >= 2^31
WORDS_BAD = [([0], b"word of 0"), ([0, 5, 9], b"word of 0"), ([5, 5], b"ascending"), ([300, 200, 100], b"ascending"), ([1, 2, 3, 3], b"ascending"),
             (list(range(1, 64)) + [62], b"ascending"), ([65535, 1], b"ascending")]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _refused(lib, args, word):
    rc = lib.pc_prob_truth_hist(*[args[k] for k in ORDER], None)
    assert rc == -1, (args, rc)                              # PC_E_ARG, before any HIP call (there is no device here to make one on)
    msg = lib.pc_last_error()
    assert word in msg and b"pc_prob_truth_hist" in msg, (word, msg)


# ---------------------------------------------------------------------- the entries
def test_prob_truth_hist_refuses_bad_arguments_without_gpu(built):
    for key, val, word in BAD:
        _refused(built, dict(OK, **{key: val}), word)
    for H, W in SIZE_BAD:
        _refused(built, dict(OK, H=H, W=W), b"2^31")
    _refused(built, dict(OK, F=2 ** 31 - 1, f0=2 ** 31 - 1, nf=2 ** 31 - 1), b"f0")          # f0 + nf beyond int32
    for words, word in WORDS_BAD:
        _refused(built, dict(OK, thr=(C.c_uint16 * len(words))(*words), N=len(words)), word)


def test_ws_bytes_is_host_arithmetic_and_minus_one_where_the_call_refuses(built):
    ws = built.pc_prob_truth_hist_ws_bytes
    assert ws(1, 1, 1, 1) == 4 * 4                           # one block, a 2 x 2 table
    assert ws(3, 5, 7, 19) == 3 * 40 * 4
    assert ws(40, 240, 320, 19) == 40 * 19 * 40 * 4          # 19200 groups of four at 1024 a block
    assert ws(1, 1080, 1920, 64) == 64 * 130 * 4             # the cap of 64 blocks per frame at the largest table
    assert ws(1, 1, 256 * 1024, 1) == 64 * 4 * 4 and ws(1, 1, 63 * 4096, 1) == 63 * 4 * 4
    assert ws(2 ** 31 - 1, 46340, 46340, 64) == (2 ** 31 - 1) * 64 * 130 * 4               # the largest of all: no overflow in int64
    assert ops.prob_truth_hist_ws_bytes(40, 240, 320, 19) == ws(40, 240, 320, 19)
    for bad in ((0, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, -4, -4, 1), (1, 1 << 16, 1 << 15, 1), (1, 2 ** 31 - 1, 2 ** 31 - 1, 1),
                (1, 4, 4, 0), (1, 4, 4, 65), (1, 4, 4, -1), (1, 4, 4, -2 ** 31)):
        assert ws(*bad) == -1, bad
        with pytest.raises(ValueError):
            ops.prob_truth_hist_ws_bytes(*bad)


def test_host_side_of_the_entries_under_asan_ubsan():
    """Every refusal path and the workspace arithmetic as a stand-alone program against the sanitizer build of the library (no GPU, nothing
    loaded into Python): tests/prob_hist_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/prob_hist_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "prob_hist_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_prob_truth_hist", "pc_prob_truth_hist_ws_bytes"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header)
        getattr(built, name)
    assert int(re.search(r"#define\s+PC_SWEEP_MAX_THRESHOLDS\s+(\d+)", header).group(1)) == ops.SWEEP_MAX_THRESHOLDS == 64
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\bprob_hist\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bprobhist\.hip\b", mk, re.M)


def test_constructors_keep_their_last_parameters_and_sweep_is_a_method():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"
    assert list(inspect.signature(detect.DetectEngine.sweep).parameters) == ["self", "truths", "labels", "thresholds", "videos"]
    sig = inspect.signature(detect.DetectEngine.sweep).parameters
    assert sig["thresholds"].default is None and sig["videos"].default is None
    assert list(inspect.signature(detect.DetectEngine.set_keep_probs).parameters) == ["self", "keep"]
    assert inspect.signature(detect.DetectEngine.set_keep_probs).parameters["keep"].default is True


def test_set_keep_probs_takes_a_bool_only():
    eng = detect.DetectEngine.__new__(detect.DetectEngine)   # the setter touches one field: no device is needed to see it refuse
    eng.keep_probs = False
    for bad in (None, 1, 0, "yes", 1.0, [True], np.int32(1)):
        with pytest.raises(ValueError, match="set_keep_probs"):
            eng.set_keep_probs(bad)
        assert eng.keep_probs is False
    eng.set_keep_probs()
    assert eng.keep_probs is True
    with pytest.raises(ValueError):
        eng.set_keep_probs("no")
    assert eng.keep_probs is True
    eng.set_keep_probs(False)
    assert eng.keep_probs is False
    eng.set_keep_probs(np.True_)
    assert eng.keep_probs is True


# ---------------------------------------------------------------------- the words
def test_threshold_words():
    w = detect.threshold_words([0.5])
    assert w.dtype == np.uint16 and w.tolist() == [32768]    # seg_positive: the word of a logit of +-0.0
    assert detect.threshold_words([1.0]).tolist() == [65535]
    assert detect.threshold_words([1.0 / 65535.0]).tolist() == [1]
    assert detect.threshold_words([1e-9]).tolist() == [1] and detect.threshold_words([0.50001]).tolist() == [32769]
    d = detect.threshold_words()
    assert d.tolist() == detect.threshold_words(None).tolist() == detect.threshold_words([k / 20.0 for k in range(1, 20)]).tolist()
    assert d.size == 19 and d[9] == 32768 and d[0] == 3277 and d[18] == 62259 and (np.diff(d.astype(np.int64)) > 0).all()
    # the ceiling of the float64 product, as specified: within one word above t
    for k, t in enumerate(detect.DEFAULT_SWEEP):
        q = int(d[k])
        assert q == math.ceil(t * 65535.0) and 0.0 <= q / 65535.0 - t + 1e-15 < 1.0 / 65535.0
    assert detect.threshold_words(np.linspace(0.01, 1.0, 64)).size == 64
    assert detect.threshold_words(np.array([0.25, 0.75], np.float32)).tolist() == [16384, 49152]
    for bad in ([0.0], [-0.1], [1.0 + 1e-12], [2], [float("nan")], [0.2, float("nan")], [float("inf")], [], [[0.5]], 0.5, np.linspace(0.01, 1.0, 65),
                [0.5, 0.5], [0.6, 0.4], [0.5, 0.5 + 1e-7], ["a"], [None]):
        with pytest.raises(ValueError, match="threshold_words"):
            detect.threshold_words(bad)


# ---------------------------------------------------------------------- the counts
def _maps(rng, shape, words):
    """Random uint16 maps that hold every word, its two neighbours, 0 and 65535, and a truth of noise with one empty frame."""
    F, H, W = shape
    special = np.unique(np.clip(np.concatenate([np.asarray(words, np.int64) + d for d in (-1, 0, 1)] + [np.array([0, 65535])]), 0, 65535))
    prob = rng.integers(0, 65536, shape).astype(np.uint16)
    pick = rng.random(shape) < 0.5
    prob[pick] = special[rng.integers(0, special.size, int(pick.sum()))].astype(np.uint16)
    truth = (rng.random(shape) < 0.3).astype(np.uint8) * rng.integers(1, 256, shape).astype(np.uint8)
    truth[F - 1] = 0
    return prob, truth


@pytest.mark.parametrize("words", [[1], [65535], [32768], [1, 2, 3], list(range(1, 65)), [3277, 32768, 62259], [1, 65535],
                                   detect.threshold_words().tolist(), sorted(set(np.random.default_rng(3).integers(1, 65536, 64).tolist()))])
def test_sweep_counts_are_the_counts_of_each_thresholds_mask(words):
    rng = np.random.default_rng(len(words) + words[0])
    prob, truth = _maps(rng, (3, 9, 11), words)
    h = ref.hist(prob, truth, words)
    assert h.shape == (3, 2, len(words) + 1) and (h.reshape(3, -1).sum(1) == 99).all()
    got = detect.sweep_counts(h)
    assert got.dtype == np.int64 and got.shape == (len(words), 3, 3)
    assert np.array_equal(got, ref.brute_counts(prob, truth, words))
    assert np.array_equal(got, ref.sweep_counts(h))
    for k, w in enumerate(words):                            # and threshold by threshold what score() counts for that mask
        table = cref.crosstab((prob >= w).astype(np.uint8), truth, 1, 1)
        assert np.array_equal(got[k], detect.crosstab_counts(table))


def test_one_word_at_a_half_is_the_crosstab_of_the_mask():
    rng = np.random.default_rng(11)
    prob, truth = _maps(rng, (4, 7, 13), [32768])
    h = ref.hist(prob, truth, [32768])
    table = cref.crosstab((prob >= 32768).astype(np.uint8), truth, 1, 1)
    assert np.array_equal(detect.sweep_counts(h)[0], detect.crosstab_counts(table))
    binary = cref.crosstab((prob >= 32768).astype(np.uint8), (truth != 0).astype(np.uint8), 1, 1)
    assert np.array_equal(h, binary[:, :2, :2].transpose(0, 2, 1))           # hist[f, t, b] = table[f, p = b, a = t]
    for bad in (np.zeros((3, 2), np.int32), np.zeros((3, 3, 4), np.int32), np.zeros((3, 2, 1), np.int32)):
        with pytest.raises(ValueError):
            detect.sweep_counts(bad)


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k       # bit for bit, NaNs by position


def test_sweep_pass_at_one_threshold_is_score_pass_on_the_matching_tables():
    rng = np.random.default_rng(5)
    C_ = 6
    words = detect.threshold_words()
    vids, labels, predicted = [], [3, 1, 4, 1, 5], [3, 0, 4, 1, 2]
    for F in (2, 8, 17, 5, 3):                               # (the last frame of each holds no truth)
        vids.append(_maps(rng, (F, 6, 10), words))
    vids[3] = (vids[3][0], np.zeros_like(vids[3][1]))        # a video without any truth: skipped by both
    hists = [ref.hist(p, t, words) for p, t in vids]
    sw = detect.sweep_pass(hists, labels, predicted, C_, words)
    assert isinstance(sw, detect.SweepScore) and sw.n_skipped == 1 and len(sw.results) == 19 and len(sw.videos) == 5
    assert sw.fmAP.shape == sw.vmAP.shape == (19, evalmetrics.N_THR) and sw.fmAP.dtype == np.float64 and sw.pixel.shape == (19, 3)
    assert np.array_equal(sw.words, words) and np.allclose(sw.thresholds, words / 65535.0, rtol=0, atol=1e-15)
    for k, w in enumerate(words.tolist()):
        tables = [cref.crosstab((p >= w).astype(np.uint8), t, 1, 1) for p, t in vids]
        ps = detect.score_pass(tables, labels, predicted, C_)
        _same(sw.results[k], ps.result)
        assert np.array_equal(sw.fmAP[k], ps.result["fmAP"], equal_nan=True) and np.array_equal(sw.vmAP[k], ps.result["vmAP"], equal_nan=True)
        one = detect.sweep_pass([ref.hist(p, t, [w]) for p, t in vids], labels, predicted, C_, [w])
        _same(one.results[0], ps.result)
        # pixels over every frame of every scored video
        scored = [(p, t) for p, t in vids if t.any()]
        tp = sum(int(((p >= w) & (t != 0)).sum()) for p, t in scored)
        fp = sum(int(((p >= w) & (t == 0)).sum()) for p, t in scored)
        fn = sum(int(((p < w) & (t != 0)).sum()) for p, t in scored)
        assert sw.pixel[k].tolist() == [tp, fp, fn] == one.pixel[0].tolist()
    assert all(np.array_equal(a, b) for a, b in zip(sw.videos, hists))
    empty = detect.sweep_pass([], [], [], C_, words)
    assert empty.videos == [] and empty.n_skipped == 0 and len(empty.results) == 19 and empty.results[0]["n_correct"] == 0 and not empty.pixel.any()
    with pytest.raises(ValueError):
        detect.sweep_pass(hists, labels, predicted, C_, words[:5])


def test_best_is_the_first_largest_and_ignores_nan():
    def score(col10_f, col10_v):
        n = len(col10_f)
        res = []
        for a, b in zip(col10_f, col10_v):
            f, v = np.zeros(evalmetrics.N_THR), np.zeros(evalmetrics.N_THR)
            f[10], v[10], f[4] = a, b, 1.0 - (0.0 if np.isnan(a) else a)
            res.append(dict(fmAP=f, vmAP=v))
        return detect.SweepScore(np.linspace(0.1, 0.9, n), np.arange(1, n + 1), res, np.zeros((n, 3)), [], 0)
    nan = float("nan")
    s = score([0.1, 0.7, 0.7, 0.3], [0.9, nan, 0.2, 0.9])
    assert s.best() == 1 and s.best("fmAP", 0.5) == 1 and s.best(metric="vmAP") == 0 and s.best("fmAP", iou=0.2) == 0
    assert score([nan, 0.2, nan, 0.2], [nan] * 4).best() == 1
    with pytest.raises(ValueError, match="NaN"):
        score([nan, 0.2, nan, 0.2], [nan] * 4).best("vmAP")
    for kw in (dict(metric="accuracy"), dict(iou=1.0), dict(iou=-0.05), dict(iou=0.52), dict(iou="x"), dict(iou=nan)):
        with pytest.raises(ValueError):
            s.best(**kw)
    assert s.best(iou=0.0) == 0 and s.best(iou=0.95) == 0      # all equal there: the first
