"""CPU: what the detection output decides on the host, without a GPU.  link_tubes, the clip coverage DetectEngine relies on (every frame of a
video in exactly one clip), and the four C entry points behind it (pc_clips_from_u8, pc_detect_frames, pc_detect_frames_ws_bytes,
pc_video_class) refusing every bad argument before any HIP call -- through capi, and as a stand-alone program under ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, evalstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _records(counts):
    """counts -> (counts, boxes, scores): frame t with count > 0 has the box (t, t + 1, t + 3, t + 5) and the score 0.5 + t / 100."""
    counts = np.asarray(counts, np.int32)
    F = counts.size
    boxes = np.zeros((F, 4), np.int32)
    scores = np.zeros(F, np.float32)
    for t in range(F):
        if counts[t] > 0:
            boxes[t] = (t, t + 1, t + 3, t + 5)
            scores[t] = 0.5 + t / 100.0
    return counts, boxes, scores


def test_link_tubes_empty_and_single_frames():
    assert detect.link_tubes([], np.zeros((0, 4), np.int32), []) == []
    assert detect.link_tubes(*_records([0])) == []
    assert detect.link_tubes(*_records([0, 0, 0])) == []
    c, b, s = _records([7])
    (t0, t1, bx, sc), = detect.link_tubes(c, b, s)
    assert (t0, t1) == (0, 0) and np.array_equal(bx, b[0:1]) and sc == float(np.float64(s[0]))


def test_link_tubes_all_frames_detected_is_one_tube():
    c, b, s = _records([3, 1, 9, 2, 5])
    (t0, t1, bx, sc), = detect.link_tubes(c, b, s)
    assert (t0, t1) == (0, 4) and np.array_equal(bx, b) and bx is not b
    assert sc == float(np.mean(s.astype(np.float64)))


def test_link_tubes_two_runs_and_the_gap_between_them():
    c, b, s = _records([0, 4, 4, 0, 0, 4, 4, 4, 0])              # runs 1..2 and 5..7, two empty frames between
    tubes = detect.link_tubes(c, b, s)
    assert [(t[0], t[1]) for t in tubes] == [(1, 2), (5, 7)]
    assert np.array_equal(tubes[0][2], b[1:3]) and np.array_equal(tubes[1][2], b[5:8])
    assert tubes[0][3] == float(np.mean(s[1:3].astype(np.float64))) and tubes[1][3] == float(np.mean(s[5:8].astype(np.float64)))
    assert [(t[0], t[1]) for t in detect.link_tubes(c, b, s, max_gap=1)] == [(1, 2), (5, 7)]       # one frame short of the gap
    (t0, t1, bx, sc), = detect.link_tubes(c, b, s, max_gap=2)                                       # exactly the gap
    assert (t0, t1) == (1, 7) and np.array_equal(bx, b[1:8])
    assert not bx[2:4].any()                                                                        # the bridged frames keep their empty box
    det = np.array([1, 2, 5, 6, 7])
    assert sc == float(np.mean(s[det].astype(np.float64)))                                          # the mean over the detected frames only
    assert sc != float(np.mean(s[1:8].astype(np.float64)))
    assert [(t[0], t[1]) for t in detect.link_tubes(c, b, s, max_gap=50)] == [(1, 7)]               # never beyond the first / last detection


def test_link_tubes_min_pixels_drops_small_frames():
    c, b, s = _records([5, 2, 5, 5, 1, 0, 9])
    assert [(t[0], t[1]) for t in detect.link_tubes(c, b, s)] == [(0, 4), (6, 6)]
    tubes = detect.link_tubes(c, b, s, min_pixels=3)
    assert [(t[0], t[1]) for t in tubes] == [(0, 0), (2, 3), (6, 6)]
    assert tubes[1][3] == float(np.mean(s[2:4].astype(np.float64)))
    (t0, t1, bx, sc), (u0, u1, _b, _s) = detect.link_tubes(c, b, s, min_pixels=3, max_gap=1)
    assert (t0, t1, u0, u1) == (0, 3, 6, 6)
    assert np.array_equal(bx[1], b[1]) and bx[1].any()            # a bridged frame below min_pixels keeps the box it has
    assert sc == float(np.mean(s[[0, 2, 3]].astype(np.float64)))
    assert detect.link_tubes(c, b, s, min_pixels=10) == []
    for bad in (dict(min_pixels=0), dict(max_gap=-1)):
        with pytest.raises(ValueError):
            detect.link_tubes(c, b, s, **bad)
    with pytest.raises(ValueError):
        detect.link_tubes(c, b[:3], s)


def test_detection_tubes_are_link_tubes_of_its_records():
    c, b, s = _records([0, 4, 0, 4])
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), c, b, s, None)
    got, want = d.tubes(max_gap=1), detect.link_tubes(c, b, s, max_gap=1)
    assert len(got) == len(want) == 1 and got[0][:2] == want[0][:2] == (1, 3) and got[0][3] == want[0][3]


@pytest.mark.parametrize("F", (1, 8, 15, 16, 17, 31, 40))
def test_the_clips_of_an_unlabelled_video_cover_every_frame_exactly_once(F):
    starts = evalstep.clip_starts(F, np.ones(F, np.int32))
    assert starts and all(0 <= s < F for s in starts) and len(set(starts)) == len(starts)
    seen = np.zeros(F + 64, np.int32)
    for s in starts:
        for k in range(8):
            seen[s + 2 * k] += 1
    assert (seen[:F] == 1).all(), (F, starts, seen[:F])
    # no clip without a real frame: one fewer start would leave a frame uncovered
    assert len(starts) == len([i + j for i in range(0, F, 16) for j in (0, 1) if i + j < F])


def test_collect_launches_are_the_slices_every_route_cut_for_itself():
    """detect.collect_launches against the four formula sets DetectEngine._collect held, one per route (hop, working frame, views, centre crop
    with V = 1), written out as they stood.  n up to 70: three launches, where the engine's tests (bs <= 32) reach only the first."""
    per = 8 * 8 * 8
    for n in range(1, 71):
        for V in (1, 2, 3, 4):
            for slot, first, row0 in ((0, 0, 0), (3, 0, 7), (0, 5, 0), (11, 40, 129), (64, 33, 250)):
                hop, work, views, centre = [], [], [], []
                for q in range(0, n, 32):
                    k = min(32, n - q)
                    hop.append(((slot + q) * per, (slot + q + (V - 1) * n + k) * per, first + q, first + q + k, first + q == 0))
                for q in range(0, n, 32):
                    k = min(32, n - q)
                    work.append(((slot + q) * per, (slot + q + (V - 1) * n + k) * per, first + q, first + q + k, row0 + (first + q) * V))
                for q in range(0, n, 32):
                    k = min(32, n - q)
                    views.append(((slot + q) * per, (slot + q + (V - 1) * n + k) * per, first + q, first + q + k, row0 + (first + q) * V))
                for q in range(0, n, 32):
                    k = min(32, n - q)
                    centre.append(((slot + q) * per, (slot + q + k) * per, first + q, first + q + k, row0 + first + q))
                got = detect.collect_launches(n, V, slot, first, row0, per)
                assert len(got) == (n + 31) // 32 and all(s1 - s0 <= 32 for _lo, _hi, s0, s1, _row in got)
                assert got == work == views, (n, V, slot, first, row0)
                assert [g[:4] + (g[2] == 0,) for g in got] == hop, (n, V, slot, first, row0)          # cover: with the video's first clip
                if V == 1:
                    assert got == centre, (n, slot, first, row0)


def _refusals(lib):
    """(entry, argument order, good arguments, [(key, bad value, word of the message)])."""
    vp = C.c_void_p
    st = (C.c_int32 * 32)(*range(32))
    neg = (C.c_int32 * 32)(*([0] * 31 + [-1]))
    crop = [("F", 0, b"outside"), ("h0", 5, b"outside"), ("w0", 5, b"outside"), ("h0", -1, b"outside"), ("w0", -1, b"outside"), ("S", 0, b"outside"),
            ("S", 16, b"outside"), ("H", 9, b"outside"), ("W", 9, b"outside")]
    clips = [("n", 0, b"clips outside"), ("n", 33, b"clips outside"), ("n", -1, b"clips outside"), ("f_skip", 0, b"f_skip"), ("f_skip", -2, b"f_skip"),
             ("starts", neg, b"negative")]
    cut = (lib.pc_clips_from_u8, ("video", "F", "H", "W", "h0", "w0", "S", "starts", "n", "f_skip", "data"),
           dict(video=vp(64), F=20, H=12, W=12, h0=2, w0=2, S=8, starts=st, n=2, f_skip=2, data=vp(64)),
           [(k, None, b"null") for k in ("video", "starts", "data")] + crop + clips + [("data", vp(68), b"16-byte")])
    frames = (lib.pc_detect_frames, ("logits", "F", "H", "W", "h0", "w0", "S", "starts", "n", "f_skip", "row0", "mask", "rec", "ws"),
              dict(logits=vp(64), F=20, H=12, W=12, h0=2, w0=2, S=8, starts=st, n=2, f_skip=2, row0=0, mask=vp(64), rec=vp(64), ws=vp(64)),
              [(k, None, b"null") for k in ("logits", "starts", "rec", "ws")] + crop + clips +
              [("S", 6, b"multiple of 4"), ("S", 2, b"multiple of 4"), ("logits", vp(68), b"16-byte"), ("logits", vp(72), b"16-byte"),
               ("ws", vp(68), b"aligned"), ("rec", vp(66), b"aligned"), ("row0", -1, b"row0")])
    cls = (lib.pc_video_class, ("scores", "n", "C", "out"), dict(scores=vp(64), n=3, C=24, out=vp(64)),
           [("scores", None, b"null"), ("out", None, b"null"), ("n", 0, b"n = 0"), ("n", -1, b"n = -1"), ("C", 0, b"C = 0"), ("C", -3, b"C = -3")])
    return cut, frames, cls


def test_bad_arguments_are_refused_without_gpu(built):
    for fn, order, ok, bad in _refusals(built):
        for key, val, word in bad:
            args = dict(ok, **{key: val})
            if key == "starts" and val is not None:
                args["n"] = 32                                   # the negative start is the last of 32
            rc = fn(*[args[k] for k in order], None)
            assert rc == -1, (fn.__name__, key, val, rc)         # PC_E_ARG, before any HIP call (there is no device here to make one on)
            assert word in built.pc_last_error(), (fn.__name__, key, val, built.pc_last_error())
    ws = built.pc_detect_frames_ws_bytes
    assert [ws(n, S) for n, S in ((0, 8), (33, 8), (-1, 8), (2, 0), (2, 6), (2, -4), (2, 32772))] == [-1] * 7
    assert ws(1, 4) == 8 * 32 and ws(3, 112) == 3 * 8 * 4 * 32 and ws(14, 224) == 14 * 8 * 13 * 32 and ws(32, 224) == 32 * 8 * 13 * 32


def test_header_binding_and_library_agree_on_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_clips_from_u8", "pc_detect_frames", "pc_detect_frames_ws_bytes", "pc_video_class"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header), name
        getattr(built, name)


def test_host_side_of_the_detect_entries_under_asan_ubsan():
    """Every refusal path of the four entries as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/detect_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/detect_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "detect_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
