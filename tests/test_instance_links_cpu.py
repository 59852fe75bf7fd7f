"""CPU: what linking per-actor tubes by mask overlap decides on the host, without a GPU.  The refusals of pc_instance_overlaps before any HIP
call -- through capi, and as a stand-alone program under ASan + UBSan --, the decoding of its record, detect.link_instance_tubes_by_mask on
overlaps from the numpy restatement (tests/instance_links_ref.py), Detection.instance_tubes(link=...) and the constructor of DetectEngine."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from picons_amd import capi, detect, ops

from tests import instance_links_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


# ---------------------------------------------------------------------- the entry
def test_instance_overlaps_refuses_bad_arguments_without_gpu(built):
    vp = C.c_void_p
    order = ("imap", "F", "H", "W", "f0", "nf", "K", "L", "out")
    ok = dict(imap=vp(65), F=4, H=12, W=12, f0=0, nf=4, K=8, L=2, out=vp(64))
    bad = [("imap", None, b"null"), ("out", None, b"null"), ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"), ("W", 0, b"outside"),
           ("W", -3, b"outside"), ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"),
           ("f0", 2 ** 31 - 1, b"f0"), ("K", 0, b"K ="), ("K", 33, b"K ="), ("K", -1, b"K ="), ("L", 0, b"L ="), ("L", 5, b"L ="), ("L", -1, b"L ="),
           ("out", vp(66), b"aligned"), ("out", vp(65), b"aligned"), ("out", vp(67), b"aligned")]
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        rc = built.pc_instance_overlaps(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                      # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error() and b"pc_instance_overlaps" in built.pc_last_error(), (key, val, built.pc_last_error())
    for H, W in ((65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2)):
        args = dict(ok, H=H, W=W)
        assert built.pc_instance_overlaps(*[args[k] for k in order], None) == -1 and b"2^31" in built.pc_last_error()


def test_host_side_of_the_entry_under_asan_ubsan():
    """Every refusal path of pc_instance_overlaps as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/instance_links_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/instance_links_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "instance_links_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    assert "pc_instance_overlaps" in capi.EXPORTS and re.search(r"\bpc_instance_overlaps\(", header)
    getattr(built, "pc_instance_overlaps")
    lags = int(re.search(r"#define\s+PC_LINK_MAX_LAGS\s+(\d+)", header).group(1))
    assert lags == ops.LINK_MAX_LAGS == ref.MAX_LAGS == 4
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^asan:.*\binstance_links\b", f.read(), re.M)


def test_decode_instance_overlaps():
    K, L, F = 2, 3, 4
    want = (np.arange(F * L * (K + 1) ** 2, dtype=np.int64) * 7919 % 70001).astype(np.int32).reshape(F, L, K + 1, K + 1)
    want[1, 2, 0, 2] = 2 ** 31 - 1
    for given in (want, want.reshape(-1), want.reshape(F, -1), torch.from_numpy(want.copy()), torch.from_numpy(want.reshape(-1).copy())):
        got = ops.decode_instance_overlaps(given, K, L)
        assert got.dtype == np.int32 and got.shape == (F, L, K + 1, K + 1) and np.array_equal(got, want)
    got = ops.decode_instance_overlaps(want, K, L)
    got[0, 0, 0, 0] += 1
    assert want[0, 0, 0, 0] == 0                             # a copy, not a view of what it was given
    with pytest.raises(ValueError):
        ops.decode_instance_overlaps(want.reshape(-1)[:-1], K, L)


def test_the_restatement_on_a_case_counted_by_hand():
    K = 2
    imap = np.array([[[1, 1, 2, 0, 255, 3]], [[1, 2, 2, 9, 0, 1]], [[0, 1, 0, 1, 1, 254]]], np.uint8)
    ov = ref.overlaps(imap, K, 3)
    assert ov.dtype == np.int32 and ov.shape == (3, 3, 3, 3)
    assert ov[0, 0].tolist() == [[1, 1, 0], [0, 1, 0], [1, 0, 0]]             # (0,0) (0,1) (1,1) - - (K,0)
    assert ov[0, 1].tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 1]]             # frame 0 against frame 2
    assert ov[1, 0].tolist() == [[0, 0, 1], [1, 0, 0], [1, 0, 0]]
    assert not ov[0, 2].any() and not ov[1, 1:].any() and not ov[2].any()     # no such later frame
    assert ref.slot_pixels(imap, K).tolist() == [[2, 1, 2], [2, 2, 1], [3, 0, 1]]


# ---------------------------------------------------------------------- the case box linking gets wrong
def _corner_maps():
    """Two 20 x 20 frames: actor A a corner open to the lower left, actor B one open to the upper right, inside A's box.  A shrinks in frame 1
    and falls to rank 1."""
    m = np.zeros((2, 20, 20), np.uint8)
    a0, b, a1 = np.zeros((20, 20), bool), np.zeros((20, 20), bool), np.zeros((20, 20), bool)
    a0[0:2, :] = True
    a0[:, 18:20] = True
    b[4:20, 0:2] = True
    b[18:20, 2:14] = True
    a1[0:2, 12:20] = True
    a1[:, 18:20] = True
    assert not (a0 & b).any() and not (a1 & b).any()
    m[0][a0], m[0][b] = 1, 2
    m[1][b], m[1][a1] = 1, 2
    return m


def test_box_linking_swaps_the_corner_actors_and_mask_linking_does_not():
    K = 2
    imap = _corner_maps()
    kept, boxes, areas = ref.instance_fields(imap, K)
    assert kept.tolist() == [2, 2] and areas.tolist() == [[76, 56], [56, 52]]
    assert boxes.tolist() == [[[0, 0, 20, 20], [0, 4, 14, 20]], [[0, 4, 14, 20], [12, 0, 20, 20]]]
    assert detect.box_iou(boxes[0, 0], boxes[1, 0]) == 0.56 and detect.box_iou(boxes[0, 0], boxes[1, 1]) == 0.40
    assert detect.box_iou(boxes[0, 1], boxes[1, 1]) == 32.0 / 352.0 < 0.3
    fs = np.array([0.5, 0.75], np.float32)
    # by box: A's tube takes B, B's own tube finds nothing, A's continuation opens a third
    by_box = detect.link_instance_tubes(kept, boxes, areas, fs)
    assert [(t[0], t[1], t[3].tolist()) for t in by_box] == [(0, 1, [76, 56]), (0, 0, [56]), (1, 1, [52])]
    # by mask: each its own
    ov = ref.overlaps(imap, K, 1)
    assert ov[0, 0].tolist() == [[0, 52, 0], [56, 0, 0], [0, 0, 0]]
    by_mask = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov)
    assert [(t[0], t[1], t[3].tolist()) for t in by_mask] == [(0, 1, [76, 52]), (0, 1, [56, 56])]
    assert by_mask[0][2].tolist() == [[0, 0, 20, 20], [12, 0, 20, 20]] and by_mask[1][2].tolist() == [[0, 4, 14, 20]] * 2
    assert by_mask[0][4] == by_mask[1][4] == float(np.mean(fs.astype(np.float64)))
    # A's IoU is 52 / 76: a threshold above it opens new tubes instead, one at it does not
    assert len(detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, iou_min=52.0 / 76.0)) == 2
    assert len(detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, iou_min=0.69)) == 3
    # through Detection
    flags = np.zeros(2, np.int32)
    d = detect.Detection(3, 0.7, np.zeros(24, np.float32), areas.sum(1), boxes[:, 0], fs, None,
                         inst=(kept.copy(), kept, flags, areas, boxes, np.zeros((2, K), np.int32)), inst_overlaps=ov)
    assert [t[3].tolist() for t in d.instance_tubes()] == [t[3].tolist() for t in d.instance_tubes(link="box")] == [[76, 56], [56], [52]]
    assert [t[3].tolist() for t in d.instance_tubes(link="mask")] == [[76, 52], [56, 56]]


# ---------------------------------------------------------------------- gaps, overflow frames, slot K, scores
def _blob_video(F, on, K=2, L=1, size=12):
    """One 4 x 5 blob in the frames `on`, nothing in the others -> (imap, kept, boxes, areas, frame scores, overlaps)."""
    imap = np.zeros((F, size, size), np.uint8)
    for f in on:
        imap[f, 3:7, 2:7] = 1
    kept, boxes, areas = ref.instance_fields(imap, K)
    return imap, kept, boxes, areas, (0.5 + np.arange(F) / 100.0).astype(np.float32), ref.overlaps(imap, K, L)


@pytest.mark.parametrize("d", (1, 2, 3))
def test_max_gap_of_l_minus_1_bridges_with_that_lags_record_and_one_more_is_refused(d):
    L = d + 1
    _imap, kept, boxes, areas, fs, ov = _blob_video(d + 3, (0, d + 1, d + 2), L=L)
    assert ov[0, d, 0, 0] == 20 and not ov[0, :d].any()                        # only lag d joins frame 0 and frame d + 1
    (t0, t1, bx, ar, score), = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, max_gap=L - 1)
    assert (t0, t1) == (0, d + 2) and ar.tolist() == [20] + [0] * d + [20, 20] and not bx[1:d + 1].any()
    assert score == float(np.mean(fs[[0, d + 1, d + 2]].astype(np.float64)))                # the bridged frames do not count
    # the record of lag d decides it: with that one cleared the tube ends, whatever the lags below it say
    cleared = ov.copy()
    cleared[0, d] = 0
    cleared[0, :d] = 99
    assert [(t[0], t[1]) for t in detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, cleared, max_gap=L - 1)] == [(0, 0), (d + 1, d + 2)]
    # a smaller gap closes the tube; a larger one has no record
    assert [(t[0], t[1]) for t in detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, max_gap=d - 1)] == [(0, 0), (d + 1, d + 2)]
    with pytest.raises(ValueError, match="max_gap"):
        detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, max_gap=L)
    assert len(detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, max_gap=L - 1, min_len=4)) == 0


def test_a_frame_with_the_overflow_flag_links_through_slot_k():
    """Frame 1 overflowed: its map is 255 on all foreground, the substitute gave it one instance with the frame's count.  The tube of the
    actor that holds most of that foreground goes through it; the other actor's tube ends."""
    K = 2
    imap = np.zeros((3, 16, 16), np.uint8)
    imap[0, 2:10, 2:8], imap[0, 12:14, 10:14] = 1, 2                            # 48 and 8 pixels
    imap[1, 2:10, 2:8], imap[1, 12:14, 10:14] = 255, 255                       # the same foreground, unlabelled
    imap[2, 2:10, 2:8], imap[2, 12:14, 10:14] = 1, 2
    kept, boxes, areas = ref.instance_fields(imap, K)
    flags = np.array([0, 1, 0], np.int32)
    counts = np.array([56, 56, 56], np.int32)
    fboxes = np.array([[2, 2, 14, 14]] * 3, np.int32)
    assert kept.tolist() == [2, 0, 2]
    _n, kept, flags, areas, boxes, _first = detect.substitute_overflow(counts, fboxes, 1, (kept.copy(), kept, flags, areas, boxes, np.zeros((3, K), np.int32)))
    assert kept.tolist() == [2, 1, 2] and areas[1].tolist() == [56, 0]
    ov = ref.overlaps(imap, K, 1)
    assert ov[0, 0].tolist() == [[0, 0, 48], [0, 0, 8], [0, 0, 0]] and ov[1, 0].tolist() == [[0, 0, 0], [0, 0, 0], [48, 8, 0]]
    fs = np.array([0.5, 0.6, 0.7], np.float32)
    tubes = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, flags)
    # 48 / (48 + 56 - 48) = 0.857 for the large actor, 8 / 56 for the small one; back out of the frame the same way
    assert [(t[0], t[1], t[3].tolist()) for t in tubes] == [(0, 2, [48, 56, 48]), (0, 0, [8]), (2, 2, [8])]
    # without the flags the frame's instance is read as rank 0, which its map does not hold: nothing links
    assert [(t[0], t[1]) for t in detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov)] == [(0, 0), (0, 0), (1, 1), (2, 2), (2, 2)]
    with pytest.raises(ValueError, match="flags"):
        detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, flags[:2])


def test_slot_k_of_a_frame_that_did_not_overflow_links_nothing():
    """Frame 1 holds the actor's pixels as 255 -- foreground beyond the K kept instances -- and a small instance elsewhere: the record has a
    large cell [0][K], and it is not looked at."""
    K = 1
    imap = np.zeros((2, 12, 12), np.uint8)
    imap[0, 2:8, 2:8] = 1
    imap[1, 2:8, 2:8], imap[1, 10:12, 0:4] = 255, 1
    kept, boxes, areas = ref.instance_fields(imap, K)
    ov = ref.overlaps(imap, K, 1)
    assert ov[0, 0].tolist() == [[0, 36], [0, 0]]
    fs = np.array([0.5, 0.6], np.float32)
    for flags in (None, np.zeros(2, np.int32), np.array([2, 4], np.int32)):      # bit 0 alone says overflow
        tubes = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, flags, iou_min=0.0 if flags is None else 0.3)
        if flags is None:
            assert [(t[0], t[1], t[3].tolist()) for t in tubes] == [(0, 1, [36, 8])]      # iou_min = 0 takes an IoU of 0, as by box
        else:
            assert [(t[0], t[1], t[3].tolist()) for t in tubes] == [(0, 0, [36]), (1, 1, [8])]


def test_inst_scores_follow_the_instance_as_in_link_instance_tubes():
    """The corner actors over four frames, their ranks swapping every frame; A scores 0.9 + t / 100, B 0.6 - t / 100."""
    K = 2
    two = _corner_maps()
    imap = np.stack([two[0], two[1], two[0], two[1]])
    kept, boxes, areas = ref.instance_fields(imap, K)
    sc = np.zeros((4, K), np.float64)
    for t in range(4):
        a_rank = t % 2
        sc[t, a_rank], sc[t, 1 - a_rank] = 0.9 + t / 100.0, 0.6 - t / 100.0
    fs = np.array([0.5, 0.6, 0.7, 0.8], np.float32)
    ov = ref.overlaps(imap, K, 1)
    tubes = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, inst_scores=sc)
    assert [(t[0], t[1], t[3].tolist()) for t in tubes] == [(0, 3, [76, 52, 76, 52]), (0, 3, [56, 56, 56, 56])]
    assert tubes[0][4] == float(np.mean([0.9 + t / 100.0 for t in range(4)])) and tubes[1][4] == float(np.mean([0.6 - t / 100.0 for t in range(4)]))
    plain = detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov)
    assert [(t[0], t[1], t[2].tolist(), t[3].tolist()) for t in plain] == [(t[0], t[1], t[2].tolist(), t[3].tolist()) for t in tubes]
    assert plain[0][4] == plain[1][4] == float(np.mean(fs.astype(np.float64)))
    with pytest.raises(ValueError, match="inst_scores"):
        detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, inst_scores=sc[:, :1])


def test_shape_mismatches_and_bad_arguments_are_value_errors():
    _imap, kept, boxes, areas, fs, ov = _blob_video(3, (0, 1, 2), K=2, L=2)
    assert len(detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, max_gap=1)) == 1
    assert detect.link_instance_tubes_by_mask(np.zeros(0, np.int32), np.zeros((0, 2, 4)), np.zeros((0, 2)), np.zeros(0), np.zeros((0, 1, 3, 3))) == []
    for bad in (ov[:2], ov[:, :, :2], ov[:, :, :, :2], ov.reshape(3, -1), ov[:, :0], np.zeros((3, 2, 4, 4), np.int32)):
        with pytest.raises(ValueError, match="overlaps"):
            detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, bad)
    for kw in (dict(iou_min=1.5), dict(iou_min=-0.1), dict(max_gap=-1), dict(min_len=0)):
        with pytest.raises(ValueError):
            detect.link_instance_tubes_by_mask(kept, boxes, areas, fs, ov, **kw)
    with pytest.raises(ValueError):
        detect.link_instance_tubes_by_mask(kept, boxes, areas, fs[:2], ov)
    with pytest.raises(ValueError):
        detect.link_instance_tubes_by_mask(kept, boxes, areas[:, :1], fs, ov)


# ---------------------------------------------------------------------- Detection and the engine's constructor
def _detection(**kw):
    z = np.zeros(2, np.int32)
    return detect.Detection(3, 0.7, np.zeros(24, np.float32), z, np.zeros((2, 4), np.int32), np.zeros(2, np.float32), None, **kw)


def test_detection_default_and_its_refusals():
    z = np.zeros(2, np.int32)
    inst = (z, z, z, np.zeros((2, 3), np.int32), np.zeros((2, 3, 4), np.int32), np.zeros((2, 3), np.int32))
    assert _detection().inst_overlaps is None and _detection(inst=inst).inst_overlaps is None
    params = inspect.signature(detect.Detection.__init__).parameters
    assert list(params)[-1] == "inst_overlaps" and params["inst_overlaps"].default is None              # trailing: no earlier argument moved
    tubes = inspect.signature(detect.Detection.instance_tubes).parameters
    assert list(tubes) == ["self", "iou_min", "max_gap", "min_len", "link"] and tubes["link"].default == "box"
    d = _detection(inst=inst)
    assert d.instance_tubes() == [] == d.instance_tubes(link="box")
    with pytest.raises(ValueError, match="overlaps"):
        d.instance_tubes(link="mask")
    for link in ("iou", "", None, "Mask"):
        with pytest.raises(ValueError, match="link"):
            d.instance_tubes(link=link)
    with pytest.raises(ValueError, match="instances"):
        _detection().instance_tubes(link="mask")
    d = _detection(inst=inst, inst_overlaps=np.zeros((2, 1, 4, 4), np.int32))
    assert d.instance_tubes(link="mask") == [] and d.inst_overlaps.shape == (2, 1, 4, 4)
    with pytest.raises(ValueError, match="max_gap"):
        d.instance_tubes(max_gap=1, link="mask")
    for bad in (np.zeros((2, 1, 3, 3), np.int32), np.zeros((3, 1, 4, 4), np.int32), np.zeros((2, 16), np.int32)):
        with pytest.raises(ValueError, match="inst_overlaps"):
            _detection(inst=inst, inst_overlaps=bad)
    with pytest.raises(ValueError, match="inst_overlaps"):
        _detection(inst_overlaps=np.zeros((2, 1, 4, 4), np.int32))                                    # overlaps without instances


def test_default_instance_tubes_is_todays_result():
    """The crossing actors of tests/test_instance_scores_cpu.py: instance_tubes() with and without overlaps in the detection, and with
    link="box", is link_instance_tubes' result."""
    K, frames = 3, []
    for t in range(7):
        A, B = ((4 * t, 0, 4 * t + 10, 10), 100 - 10 * t), ((24 - 4 * t, 6, 34 - 4 * t, 16), 50 + 10 * t)
        frames.append([A, B] if A[1] >= B[1] else [B, A])
    kept, boxes, areas = np.zeros(7, np.int32), np.zeros((7, K, 4), np.int32), np.zeros((7, K), np.int32)
    for t, fr in enumerate(frames):
        kept[t] = len(fr)
        for r, (b, a) in enumerate(fr):
            boxes[t, r], areas[t, r] = b, a
    fs = (0.5 + np.arange(7) / 100.0).astype(np.float32)
    inst = (kept.copy(), kept, np.zeros(7, np.int32), areas, boxes, np.zeros((7, K), np.int32))
    want = detect.link_instance_tubes(kept, boxes, areas, fs, 0.3, 1, 2)
    assert [(t[0], t[1]) for t in want] == [(0, 6), (0, 6)]
    for ov in (None, np.zeros((7, 2, K + 1, K + 1), np.int32)):
        d = detect.Detection(3, 0.7, np.zeros(24, np.float32), areas[:, 0], boxes[:, 0], fs, None, inst=inst, inst_overlaps=ov)
        for got in (d.instance_tubes(0.3, 1, 2), d.instance_tubes(max_gap=1, min_len=2, link="box")):
            assert [(t[0], t[1], t[2].tolist(), t[3].tolist(), t[4]) for t in got] == [(t[0], t[1], t[2].tolist(), t[3].tolist(), t[4]) for t in want]


def test_constructor_refusals_and_the_default_is_off():
    for kw in (dict(instance_links=1), dict(instance_links=4, instances=0), dict(instance_links=2, instances=0, instance_maps=True)):
        with pytest.raises(ValueError, match="instances"):
            detect.DetectEngine(bs=3, hw=112, device="no-such-device:0", **kw)           # before any device is touched
    for L in (-1, 5, 100):
        with pytest.raises(ValueError, match="instance_links"):
            detect.DetectEngine(bs=3, hw=112, device="no-such-device:0", instances=8, instance_links=L)
    assert inspect.signature(detect.DetectEngine.__init__).parameters["instance_links"].default == 0
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert inspect.signature(detect.link_instance_tubes_by_mask).parameters["inst_flags"].default is None
    assert list(inspect.signature(detect.link_instance_tubes_by_mask).parameters) == [
        "inst_kept", "inst_boxes", "inst_areas", "frame_scores", "overlaps", "inst_flags", "iou_min", "max_gap", "min_len", "inst_scores"]
    assert list(inspect.signature(detect.link_instance_tubes).parameters) == [
        "inst_kept", "inst_boxes", "inst_areas", "frame_scores", "iou_min", "max_gap", "min_len", "inst_scores"]
