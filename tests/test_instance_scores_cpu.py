"""CPU: what the per-instance confidence decides on the host, without a GPU.  The refusals of pc_frame_probs and pc_instance_scores before any
HIP call -- through capi, and as a stand-alone program under ASan + UBSan --, the decoding of the score record, the host scoring
(detect.score_instances), link_instance_tubes with per-instance scores, and the constructor of DetectEngine."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from picons_amd import capi, detect, ops

from tests import instance_scores_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


# ---------------------------------------------------------------------- the entries
def test_frame_probs_refuses_bad_arguments_without_gpu(built):
    vp, i32p = C.c_void_p, lambda *v: (C.c_int32 * len(v))(*v)
    order = ("logits", "F", "H", "W", "S", "views", "V", "view_stride", "starts", "n", "f_skip", "prob")
    ok = dict(logits=vp(64), F=20, H=12, W=16, S=8, views=i32p(0, 0, 0, 4, 8, 1), V=2, view_stride=2, starts=i32p(0, 1), n=2, f_skip=2, prob=vp(64))
    assert "row0" not in order and "rec" not in order and "ws" not in order
    bad = [("logits", None, b"null"), ("views", None, b"null"), ("starts", None, b"null"), ("prob", None, b"null"),
           ("F", 0, b"outside"), ("H", 0, b"outside"), ("W", -3, b"outside"), ("S", 0, b"outside"), ("S", 16, b"outside"), ("S", 32772, b"outside"),
           ("S", 6, b"multiple of 4"), ("V", 0, b"V ="), ("V", 33, b"V ="), ("n", 0, b"n ="), ("n", 33, b"n ="), ("view_stride", 1, b"view_stride"),
           ("f_skip", 0, b"f_skip"), ("logits", vp(68), b"16-byte"), ("prob", vp(65), b"2-byte"), ("prob", vp(67), b"2-byte"),
           ("views", i32p(0, 0, 0, 5, 8, 0), b"view 1"), ("views", i32p(0, -1, 0, 4, 8, 1), b"view 0"), ("views", i32p(0, 0, 0, 4, 9, 1), b"view 1"),
           ("views", i32p(0, 0, 2, 4, 8, 1), b"flip"), ("starts", i32p(0, -1), b"negative")]
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        rc = built.pc_frame_probs(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                      # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error() and b"pc_frame_probs" in built.pc_last_error(), (key, val, built.pc_last_error())
    args = dict(ok, H=65536, W=32768)
    assert built.pc_frame_probs(*[args[k] for k in order], None) == -1 and b"2^31" in built.pc_last_error()


def test_instance_scores_refuses_bad_arguments_without_gpu(built):
    vp = C.c_void_p
    order = ("imap", "prob", "F", "H", "W", "f0", "nf", "K", "out")
    ok = dict(imap=vp(65), prob=vp(64), F=4, H=12, W=12, f0=0, nf=4, K=8, out=vp(64))
    bad = [("imap", None, b"null"), ("prob", None, b"null"), ("out", None, b"null"), ("F", 0, b"outside"), ("H", 0, b"outside"), ("W", 0, b"outside"),
           ("W", -3, b"outside"), ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", 5, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
           ("K", 0, b"K ="), ("K", 33, b"K ="), ("K", -1, b"K ="), ("prob", vp(65), b"aligned"), ("out", vp(66), b"aligned"), ("out", vp(65), b"aligned")]
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        rc = built.pc_instance_scores(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)
        assert word in built.pc_last_error() and b"pc_instance_scores" in built.pc_last_error(), (key, val, built.pc_last_error())
    args = dict(ok, H=65536, W=32768)
    assert built.pc_instance_scores(*[args[k] for k in order], None) == -1 and b"2^31" in built.pc_last_error()


def test_host_side_of_both_entries_under_asan_ubsan():
    """Every refusal path of pc_frame_probs and pc_instance_scores as a stand-alone program against the sanitizer build of the library (no
    GPU, nothing loaded into Python): tests/instance_scores_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/instance_scores_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "instance_scores_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_frame_probs", "pc_instance_scores"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header), name
        getattr(built, name)
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(PC_PROB_ONE|PC_SCORE_WORDS)\s+(\d+)", header)}
    assert consts == dict(PC_PROB_ONE=ops.PROB_ONE, PC_SCORE_WORDS=ops.SCORE_WORDS) == dict(PC_PROB_ONE=ref.ONE, PC_SCORE_WORDS=ref.WORDS)
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\binstance_scores\b", mk, re.M) and re.search(r"^HDRS\s*=.*\bviewmerge\.h\b", mk, re.M)
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "detect.hip")) as f:
        src = f.read()
    assert len(re.findall(r"\bmerge_group4\(", src)) == 2 and "__fdiv_rn(" not in src                 # both kernels call the one merge


# ---------------------------------------------------------------------- decoding and host scoring
def test_decode_instance_scores_joins_lo_and_hi_as_unsigned():
    K = 2
    sums = np.array([[4311678720, 2 ** 31 + 5, 0], [65535, 0, 2 ** 32 - 1], [(1 << 40) + (0xfedcba98), 7, 2 ** 32]], np.int64)
    npix = np.array([[65792, 40000, 0], [1, 0, 70000], [2 ** 31 - 1, 1, 65537]], np.int64)
    w = ref.words(sums, npix)
    assert w.dtype == np.int32 and w.shape == (3, 3 * (K + 1))
    assert w[0, :3].tolist() == [4311678720 - 2 ** 32, 1, 65792] and w[0, 3] < 0 and w[0, 4] == 0        # hi = 1; a lo >= 2^31 is a negative word
    assert w[1, 6:9].tolist() == [-1, 0, 70000] and w[2, 0] < 0 and w[2, 1] == 256 and w[2, 6:8].tolist() == [0, 1]
    for given in (w, w.reshape(-1), torch.from_numpy(w.copy())):
        s, n = ops.decode_instance_scores(given, K)
        assert s.dtype == np.int64 and n.dtype == np.int32 and s.shape == n.shape == (3, K + 1)
        assert np.array_equal(s, sums) and np.array_equal(n, npix)


def test_score_instances_zeros_from_kept_on_overflow_takes_slot_k_and_empty_frames():
    K = 3
    sums, npix = np.zeros((4, K + 1), np.int64), np.zeros((4, K + 1), np.int64)
    # frame 0: two kept instances, a third labelled slot that does not count (kept = 2 says so), other foreground
    sums[0], npix[0] = [65535 * 10, 32768 * 4, 999, 50000 * 3], [10, 4, 1, 3]
    # frame 1: overflow -- the map is 255 on all foreground, so slot K holds the frame; the substitute gave it one instance
    sums[1, K], npix[1, K] = 4311678720, 65792
    # frame 2: overflow, but below min_area: the substitute kept nothing.  frame 3: empty
    sums[2, K], npix[2, K] = 40000, 1
    kept, flags = np.array([2, 1, 0, 0], np.int32), np.array([0, 1, 1, 0], np.int32)
    sc, other = detect.score_instances(sums, npix, kept, flags)
    assert sc.dtype == other.dtype == np.float64 and sc.shape == (4, K) and other.shape == (4,)
    assert sc[0].tolist() == [1.0, 32768 * 4 / (65535.0 * 4), 0.0] and other[0] == 150000 / (65535.0 * 3)
    assert sc[1].tolist() == [4311678720 / (65535.0 * 65792), 0.0, 0.0] and other[1] == sc[1, 0] == 1.0
    assert not sc[2].any() and other[2] == 40000 / 65535.0
    assert not sc[3].any() and other[3] == 0.0
    assert np.isfinite(sc).all() and np.isfinite(other).all()


# ---------------------------------------------------------------------- link_instance_tubes with scores
def _video(frames, K=3):
    """frames: per frame a list of (box, area, score) in rank order -> kept [F], boxes [F,K,4], areas [F,K], frame scores [F], scores [F,K]."""
    F = len(frames)
    kept, boxes, areas, sc = np.zeros(F, np.int32), np.zeros((F, K, 4), np.int32), np.zeros((F, K), np.int32), np.zeros((F, K), np.float64)
    for t, fr in enumerate(frames):
        kept[t] = len(fr)
        for r, (b, a, s) in enumerate(fr):
            boxes[t, r], areas[t, r], sc[t, r] = b, a, s
    return kept, boxes, areas, (0.5 + np.arange(F) / 100.0).astype(np.float32), sc


def test_two_crossing_actors_keep_their_own_scores():
    """The crossing actors of tests/test_instances_cpu.py: their ranks swap on the way, so a tube's score has to follow the instance, not the
    rank.  Actor A scores 0.9 + t / 100, actor B 0.6 - t / 100."""
    frames = []
    for t in range(7):
        A, B = ((4 * t, 0, 4 * t + 10, 10), 100 - 10 * t, 0.9 + t / 100.0), ((24 - 4 * t, 6, 34 - 4 * t, 16), 50 + 10 * t, 0.6 - t / 100.0)
        frames.append([A, B] if A[1] >= B[1] else [B, A])
    k, b, a, s, sc = _video(frames)
    assert frames[0][0][2] == 0.9 and frames[-1][0][2] == 0.6 - 0.06                       # rank 0 is A first, B at the end
    tubes = detect.link_instance_tubes(k, b, a, s, inst_scores=sc)
    assert [(t[0], t[1]) for t in tubes] == [(0, 6), (0, 6)]
    assert tubes[0][4] == float(np.mean([0.9 + t / 100.0 for t in range(7)])) and tubes[1][4] == float(np.mean([0.6 - t / 100.0 for t in range(7)]))
    plain = detect.link_instance_tubes(k, b, a, s)
    assert [(t[0], t[1], t[2].tolist(), t[3].tolist()) for t in plain] == [(t[0], t[1], t[2].tolist(), t[3].tolist()) for t in tubes]     # the same linking
    assert plain[0][4] == plain[1][4] == float(np.mean(s.astype(np.float64))) != tubes[0][4]
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), a[:, 0], b[:, 0], s, None, inst=(k.copy(), k, np.zeros(7, np.int32), a, b, np.zeros((7, 3), np.int32)),
                         scores=(sc, np.zeros(7)))
    assert [t[4] for t in d.instance_tubes()] == [t[4] for t in tubes]
    with pytest.raises(ValueError):
        detect.link_instance_tubes(k, b, a, s, inst_scores=sc[:, :2])


def test_a_bridged_frame_does_not_count_and_no_scores_is_todays_value():
    box = (3, 4, 13, 14)
    k, b, a, s, sc = _video([[(box, 60, 0.9)], [(box, 60, 0.7)], [], [], [(box, 60, 0.8)], [(box, 60, 0.6)], [(box, 60, 0.5)]])
    sc[2:4] = 123.0                                                    # whatever the bridged frames' rows hold, it is not looked at
    (t0, t1, bx, ar, score), = detect.link_instance_tubes(k, b, a, s, max_gap=2, inst_scores=sc)
    assert (t0, t1) == (0, 6) and not bx[2:4].any() and score == float(np.mean([0.9, 0.7, 0.8, 0.6, 0.5]))
    for kw in (dict(), dict(max_gap=2), dict(max_gap=2, min_len=5), dict(iou_min=0.95)):
        omitted, none = detect.link_instance_tubes(k, b, a, s, **kw), detect.link_instance_tubes(k, b, a, s, inst_scores=None, **kw)
        assert [(t[0], t[1], t[4]) for t in omitted] == [(t[0], t[1], t[4]) for t in none] and omitted
    (_t0, _t1, _b, _a, today), = detect.link_instance_tubes(k, b, a, s, max_gap=2)
    assert today == float(np.mean(s[[0, 1, 4, 5, 6]].astype(np.float64)))                 # the frame scores of the detected frames, as before
    assert len(detect.link_instance_tubes(k, b, a, s, 0.3, 2, 1)) == 1                    # the positional arguments stand where they stood


# ---------------------------------------------------------------------- the engine's constructor and the default Detection
def test_constructor_refusal_and_default_fields():
    for kw in (dict(instance_scores=True), dict(instance_scores=True, instances=0), dict(instance_scores=True, instances=0, instance_maps=True)):
        with pytest.raises(ValueError, match="instances"):
            detect.DetectEngine(bs=3, hw=112, device="no-such-device:0", **kw)           # before any device is touched
    z = np.zeros(2, np.int32)
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), z, np.zeros((2, 4), np.int32), np.zeros(2, np.float32), None)
    assert d.inst_scores is d.other_score is d.probs is d.imap is d.inst_kept is None
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), z, np.zeros((2, 4), np.int32), np.zeros(2, np.float32), None,
                         inst=(z, z, z, np.zeros((2, 3), np.int32), np.zeros((2, 3, 4), np.int32), np.zeros((2, 3), np.int32)))
    assert d.inst_scores is d.other_score is d.probs is None and d.instance_tubes() == []
    import inspect
    assert inspect.signature(detect.DetectEngine.__init__).parameters["instance_scores"].default is False
