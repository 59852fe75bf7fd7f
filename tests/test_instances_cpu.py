"""CPU: what the per-frame instances decide on the host, without a GPU.  The numpy restatement the GPU tests compare against
(tests/instances_ref.py) against scipy's labelling, link_instance_tubes, the refusals of pc_frame_instances before any HIP call -- through
capi, and as a stand-alone program under ASan + UBSan -- and the refusals of DetectEngine's constructor, which come before it touches a
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, ops

from tests import instances_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


# ---------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("density", (0.05, 0.3, 0.5))
def test_restatement_equals_scipy_label_and_find_objects(conn, density):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(int(density * 100) + conn)
    structure = np.ones((3, 3), int) if conn == 8 else None
    for H, W in ((1, 1), (5, 1), (1, 9), (13, 17), (37, 53)):
        frame = (rng.random((H, W)) < density).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)
        lab, n = ndi.label(frame != 0, structure=structure)
        want = []
        for i, sl in enumerate(ndi.find_objects(lab)):
            ys, xs = np.nonzero(lab == i + 1)
            want.append((ys.size, sl[1].start, sl[0].start, sl[1].stop, sl[0].stop, int((ys * W + xs).min())))
        comps, _p, _f = ref.components(frame, conn)
        assert sorted(comps) == sorted(want) and len(comps) == n
        assert [c[5] for c in comps] == sorted(c[5] for c in comps)
        for min_area, K in ((1, 1), (1, 8), (3, 32)):
            rec, imap, n_runs = ref.frame_instances(frame, conn, min_area, K)
            big = sorted((c for c in want if c[0] >= min_area), key=lambda c: (-c[0], c[5]))
            assert tuple(rec[:4]) == (len(big), min(len(big), K), n_runs, 0)
            assert rec[4:].reshape(K, 6).tolist() == [list(c) for c in big[:K]] + [[0] * 6] * (K - min(len(big), K))
            exp = np.zeros((H, W), np.uint8)
            for c in want:
                ly, lx = divmod(c[5], W)
                exp[lab == lab[ly, lx]] = big.index(c) + 1 if c in big[:K] else 255
            assert np.array_equal(imap, exp)
            assert n_runs == sum(len(re.findall("1+", "".join("1" if v else "0" for v in row))) for row in frame)


def test_restatement_reports_overflow_past_the_cap_only():
    y, x = np.mgrid[0:64, 0:66]
    board = ((y + x) % 2 == 0).astype(np.uint8)
    assert ref.count_runs(board[:, :64]) == 2048 == ops.INST_MAX_RUNS == ref.MAX_RUNS and ref.count_runs(board) == 2112
    rec, imap, n_runs = ref.frame_instances(board, 8, 1, 4)
    assert rec.tolist() == [0, 0, 2112, 1] + [0] * 24 and np.array_equal(imap, board * 255)
    rec, _imap, _n = ref.frame_instances(board[:, :64], 8, 1, 4)
    assert rec[:4].tolist() == [1, 1, 2048, 0] and rec[4:10].tolist() == [2048, 0, 0, 64, 64, 0]


# ---------------------------------------------------------------------- link_instance_tubes
def _video(frames, K=3):
    """frames: per frame a list of (box, area) in rank order -> kept [F], boxes [F,K,4], areas [F,K], scores [F] = 0.5 + t / 100."""
    F = len(frames)
    kept, boxes, areas = np.zeros(F, np.int32), np.zeros((F, K, 4), np.int32), np.zeros((F, K), np.int32)
    for t, fr in enumerate(frames):
        kept[t] = len(fr)
        for r, (b, a) in enumerate(fr):
            boxes[t, r], areas[t, r] = b, a
    return kept, boxes, areas, (0.5 + np.arange(F) / 100.0).astype(np.float32)


def test_link_instance_tubes_empty_video_and_single_frame():
    assert detect.link_instance_tubes(np.zeros(0, np.int32), np.zeros((0, 3, 4), np.int32), np.zeros((0, 3), np.int32), []) == []
    assert detect.link_instance_tubes(*_video([[]])) == []
    assert detect.link_instance_tubes(*_video([[], [], []])) == []
    k, b, a, s = _video([[((2, 3, 8, 9), 30), ((20, 3, 28, 9), 12)]])
    (t0, t1, bx, ar, sc), (u0, u1, bx2, ar2, sc2) = detect.link_instance_tubes(k, b, a, s)
    assert (t0, t1, u0, u1) == (0, 0, 0, 0) and bx.tolist() == [[2, 3, 8, 9]] and bx2.tolist() == [[20, 3, 28, 9]]
    assert ar.tolist() == [30] and ar2.tolist() == [12] and sc == sc2 == float(np.float64(s[0]))


def test_two_actors_cross_without_swapping_when_iou_separates_them():
    """Actor A moves right along y = 0..10, actor B left along y = 6..16: their boxes overlap in the middle frames, but each one's box of the
    frame before overlaps its own next box more.  Their ranks swap on the way (the areas change), the tubes do not."""
    frames = []
    for t in range(7):
        A, B = ((4 * t, 0, 4 * t + 10, 10), 100 - 10 * t), ((24 - 4 * t, 6, 34 - 4 * t, 16), 50 + 10 * t)
        frames.append([A, B] if A[1] >= B[1] else [B, A])
    k, b, a, s = _video(frames)
    assert [f[0][1] for f in frames][:2] == [100, 90] and frames[-1][0][1] == 110          # rank 0 is A first, B at the end
    tubes = detect.link_instance_tubes(k, b, a, s)
    assert [(t[0], t[1]) for t in tubes] == [(0, 6), (0, 6)]
    assert tubes[0][2].tolist() == [[4 * t, 0, 4 * t + 10, 10] for t in range(7)] and tubes[0][3].tolist() == [100 - 10 * t for t in range(7)]
    assert tubes[1][2].tolist() == [[24 - 4 * t, 6, 34 - 4 * t, 16] for t in range(7)]
    assert detect.box_iou((12, 0, 22, 10), (12, 6, 22, 16)) > 0.0                           # the middle frame: the two actors do overlap


def test_an_iou_tie_goes_to_the_lower_rank():
    # frame 1 holds two instances mirror-symmetric about the tube's box: equal IoU, rank 0 is taken; rank 1 opens its own tube
    k, b, a, s = _video([[((10, 0, 20, 10), 50)], [((14, 0, 24, 10), 40), ((6, 0, 16, 10), 40)]])
    assert detect.box_iou(b[0, 0], b[1, 0]) == detect.box_iou(b[0, 0], b[1, 1]) >= 0.3
    tubes = detect.link_instance_tubes(k, b, a, s)
    assert [(t[0], t[1]) for t in tubes] == [(0, 1), (1, 1)]
    assert tubes[0][2][1].tolist() == [14, 0, 24, 10] and tubes[1][2][0].tolist() == [6, 0, 16, 10]
    # the higher IoU wins whatever its rank
    k, b, a, s = _video([[((10, 0, 20, 10), 50)], [((15, 0, 25, 10), 40), ((9, 0, 19, 10), 40)]])
    tubes = detect.link_instance_tubes(k, b, a, s)
    assert tubes[0][2][1].tolist() == [9, 0, 19, 10] and tubes[1][2][0].tolist() == [15, 0, 25, 10]
    # below iou_min nothing links
    assert [(t[0], t[1]) for t in detect.link_instance_tubes(k, b, a, s, iou_min=0.95)] == [(0, 0), (1, 1), (1, 1)]


def test_max_gap_bridges_exactly_and_not_one_frame_short_and_min_len_and_score():
    box = ((3, 4, 13, 14), 60)
    k, b, a, s = _video([[box], [box], [], [], [box], [box], [box]])            # two empty frames between 1 and 4
    assert [(t[0], t[1]) for t in detect.link_instance_tubes(k, b, a, s)] == [(0, 1), (4, 6)]
    assert [(t[0], t[1]) for t in detect.link_instance_tubes(k, b, a, s, max_gap=1)] == [(0, 1), (4, 6)]       # one frame short
    (t0, t1, bx, ar, sc), = detect.link_instance_tubes(k, b, a, s, max_gap=2)                                   # exactly the gap
    assert (t0, t1) == (0, 6) and not bx[2:4].any() and not ar[2:4].any() and bx[[0, 1, 4, 5, 6]].all() and ar[4] == 60
    det = np.array([0, 1, 4, 5, 6])
    assert sc == float(np.mean(s[det].astype(np.float64))) != float(np.mean(s.astype(np.float64)))            # detected frames only
    (t0, t1, _b, _a, _s), = detect.link_instance_tubes(k, b, a, s, max_gap=50)
    assert (t0, t1) == (0, 6)                                                                                   # never beyond the last detection
    assert [(t[0], t[1]) for t in detect.link_instance_tubes(k, b, a, s, min_len=3)] == [(4, 6)]
    assert detect.link_instance_tubes(k, b, a, s, min_len=4) == []
    assert [(t[0], t[1]) for t in detect.link_instance_tubes(k, b, a, s, max_gap=2, min_len=5)] == [(0, 6)]    # detected frames count, not the span
    assert detect.link_instance_tubes(k, b, a, s, max_gap=2, min_len=6) == []
    for bad in (dict(iou_min=-0.1), dict(iou_min=1.5), dict(max_gap=-1), dict(min_len=0)):
        with pytest.raises(ValueError):
            detect.link_instance_tubes(k, b, a, s, **bad)
    with pytest.raises(ValueError):
        detect.link_instance_tubes(k, b[:3], a, s)


def test_detection_instance_tubes_and_the_overflow_substitute():
    k, b, a, s = _video([[((1, 1, 5, 5), 16)], [((1, 1, 5, 5), 16)]])
    n = k.copy()
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), a[:, 0], b[:, 0], s, None, inst=(n, k, np.zeros(2, np.int32), a, b, np.zeros((2, 3), np.int32)))
    got, want = d.instance_tubes(), detect.link_instance_tubes(k, b, a, s)
    assert len(got) == len(want) == 1 and got[0][:2] == want[0][:2] == (0, 1) and got[0][4] == want[0][4]
    plain = detect.Detection(3, 0.7, np.zeros(24, np.float32), a[:, 0], b[:, 0], s, None)
    assert plain.inst_n is plain.inst_kept is plain.inst_flags is plain.inst_areas is plain.inst_boxes is plain.inst_first is plain.imap is None
    with pytest.raises(ValueError):
        plain.instance_tubes()
    # a frame whose overflow flag is set holds one instance, the frame's own count and box, and keeps its flag
    counts, boxes = np.array([5000, 40], np.int32), np.array([[2, 3, 90, 80], [1, 1, 9, 9]], np.int32)
    z = lambda *sh: np.zeros(sh, np.int32)
    flags = np.array([1, 0], np.int32)
    n, kept, fl, areas, ibox, first = detect.substitute_overflow(counts, boxes, 1, (z(2), z(2), flags, z(2, 3), z(2, 3, 4), z(2, 3)))
    assert n.tolist() == [1, 0] and kept.tolist() == [1, 0] and fl.tolist() == [1, 0] and areas.tolist() == [[5000, 0, 0], [0, 0, 0]]
    assert ibox[0].tolist() == [[2, 3, 90, 80], [0] * 4, [0] * 4] and not ibox[1].any() and first.tolist() == [[-1, 0, 0], [0, 0, 0]]


# ---------------------------------------------------------------------- the entry and the engine's constructor
def test_bad_arguments_are_refused_without_gpu(built):
    vp = C.c_void_p
    order = ("mask", "F", "H", "W", "f0", "nf", "conn", "min_area", "K", "inst", "imap")
    ok = dict(mask=vp(64), F=4, H=12, W=12, f0=0, nf=4, conn=8, min_area=1, K=8, inst=vp(64), imap=vp(64))
    bad = [("mask", None, b"null"), ("inst", None, b"null"), ("F", 0, b"outside"), ("H", 0, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"),
           ("H", 2049, b"rows"), ("W", 65536, b"columns"), ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", 5, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
           ("conn", 0, b"conn"), ("conn", 6, b"conn"), ("conn", 12, b"conn"), ("min_area", 0, b"min_area"), ("min_area", -4, b"min_area"),
           ("K", 0, b"K ="), ("K", 33, b"K ="), ("K", -1, b"K ="), ("inst", vp(66), b"aligned"), ("inst", vp(65), b"aligned")]
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        rc = built.pc_frame_instances(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                      # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error(), (key, val, built.pc_last_error())


def test_engine_constructor_refusals_come_before_any_device():
    for kw in (dict(instances=4, masks=False), dict(instances=33), dict(instances=-1), dict(instances=4, conn=6), dict(instances=4, min_area=0),
               dict(conn=5), dict(min_area=0)):
        with pytest.raises(ValueError, match="instances"):
            detect.DetectEngine(bs=3, hw=112, **kw)
    with pytest.raises(ValueError, match="masks=True"):
        detect.DetectEngine(bs=3, hw=112, instances=1, masks=False)


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    assert "pc_frame_instances" in capi.EXPORTS and re.search(r"\bpc_frame_instances\(", header)
    built.pc_frame_instances
    consts = {k: int(v) for k, v in re.findall(r"#define\s+(PC_INST_\w+)\s+(\d+)", header)}
    assert consts == dict(PC_INST_HDR=ops.INST_HDR, PC_INST_WORDS=ops.INST_WORDS, PC_INST_MAX_RUNS=ops.INST_MAX_RUNS, PC_INST_MAX_ROWS=ops.INST_MAX_ROWS)
    assert (ref.HDR, ref.WORDS, ref.MAX_RUNS) == (ops.INST_HDR, ops.INST_WORDS, ops.INST_MAX_RUNS)
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SRCS\s*=.*\binstances\.hip\b", f.read(), re.M)


def test_host_side_of_the_entry_under_asan_ubsan():
    """Every refusal path of pc_frame_instances as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/instances_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/instances_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "instances_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
