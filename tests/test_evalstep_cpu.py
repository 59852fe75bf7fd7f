"""CPU: what evalstep.EvalEngine decides on the host, without a GPU.  Clip selection and the centre crop against the oracle's restatement of the
reference's loop, the ring placement, the sequential-fp32 class vote against numpy, the synthetic uint8 videos, and the three C entry points
of csrc/evalclips.hip refusing every bad argument before any HIP call (through capi, and as a stand-alone program under ASan + UBSan)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle import evalmetrics as oe
from picons_amd import capi, evalmetrics as em, evalstep, synthetic

FRAMES = (1, 8, 15, 16, 17, 31, 40)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _truths(F, H=6, W=7):
    """Truth [F,H,W,1] uint8 by case; the crop is rows 1..4, columns 1..4 (hw = 4 of 6 x 7: margins 2 and 3, offsets 1 and 1)."""
    z = lambda: np.zeros((F, H, W, 1), np.uint8)
    last, none, outside, every, phase = z(), z(), z(), z(), z()
    last[max(F - 2, 0):, 2, 2] = 1                 # only in the last frames
    outside[:, 0, :] = 1; outside[:, :, 0] = 3     # only outside the crop: flags all zero
    every[:, 3, 4] = 255
    phase[1::2, 2, 3] = 2                          # odd frames only: the even phase of every window is dropped
    return dict(last=last, none=none, outside=outside, every=every, phase=phase)


@pytest.mark.parametrize("F", FRAMES)
def test_clip_starts_keeps_the_clips_the_reference_keeps_in_its_order(F):
    hw, H, W = 4, 6, 7
    h0, w0 = evalstep.centre_crop(H, W, hw)
    assert (h0, w0) == (1, 1)
    rng = np.random.default_rng(F)
    video = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    vc = video[:, h0:h0 + hw, w0:w0 + hw] / 255.
    for name, truth in _truths(F).items():
        tc = truth[:, h0:h0 + hw, w0:w0 + hw]
        flags = np.count_nonzero(tc.reshape(F, -1), axis=1)
        starts = evalstep.clip_starts(F, flags)
        want = oe.make_clips(vc, tc, 0)
        assert len(starts) == len(want), (name, starts)
        for s, (v, b, _l) in zip(starts, want):                     # the same clips in the same order: frame k is start + 2 k, zero past the end
            for k in range(8):
                f = s + 2 * k
                assert np.array_equal(v[k], vc[f].astype(np.float32) if f < F else np.zeros_like(v[k])), (name, s, k)
                assert np.array_equal(b[k], tc[f].astype(np.float32) if f < F else np.zeros_like(b[k])), (name, s, k)
        v2, _b2 = em.make_clips(vc, tc)                             # and what the device path of today keeps
        assert v2.shape[0] == len(starts)
        if name in ("none", "outside"):
            assert starts == []                                     # the video is skipped
        if name == "every":
            assert starts == [i + j for i in range(0, F, 16) for j in (0, 1) if i + j < F]
        if name == "phase" and F > 1:
            assert starts and all(s % 2 == 1 for s in starts)


def test_clip_starts_other_frame_skips():
    assert evalstep.clip_starts(17, np.ones(17)) == [0, 1, 16]
    assert evalstep.clip_starts(17, np.ones(17), f_skip=1) == [0, 8, 16]
    assert evalstep.clip_starts(30, np.ones(30), f_skip=3) == [0, 1, 2, 24, 25, 26]
    only = np.zeros(30); only[29] = 7
    assert evalstep.clip_starts(30, only, f_skip=3) == [26]          # 26 + 3 k reaches 29; 24 and 25 do not


@pytest.mark.parametrize("H,W,hw", [(240, 320, 224), (241, 321, 224), (120, 136, 112), (225, 224, 224), (7, 10, 4)])
def test_centre_crop_is_the_references_int_of_half_the_margin(H, W, hw):
    margin_h, margin_w = H - hw, W - hw
    assert evalstep.centre_crop(H, W, hw) == (int(margin_h / 2), int(margin_w / 2))
    h0, w0 = evalstep.centre_crop(H, W, hw)
    assert 0 <= h0 and h0 + hw <= H and 0 <= w0 and w0 + hw <= W


def test_ring_placement():
    cap, bs = 16, 3
    pos, placed = 0, []
    for rows in (5, 4, 6, 2, 13, 1, 3):
        row0, pos = evalstep.ring_place(pos, rows, cap, bs)
        placed.append((row0, rows))
        assert 0 <= row0 and row0 + rows <= cap and pos == row0 + rows           # contiguous, inside the ring
    assert placed == [(0, 5), (5, 4), (9, 6), (0, 2), (2, 13), (15, 1), (0, 3)]  # 6 fits exactly to the end; 2, and the last 3, wrap to row 0
    assert evalstep.ring_place(16, 1, cap, bs) == (0, 1)
    assert evalstep.ring_place(0, cap - bs, cap, bs) == (0, 13)
    for rows in (cap - bs + 1, cap, 100):
        with pytest.raises(ValueError):
            evalstep.ring_place(0, rows, cap, bs)
    with pytest.raises(ValueError):
        evalstep.ring_place(0, 0, cap, bs)


def test_vote_restatement_equals_numpy():
    rng = np.random.default_rng(7)
    for case in range(400):
        n, Cn = int(rng.integers(1, 33)), (21, 24)[case % 2]
        p = (rng.standard_normal((n, Cn)) * 10.0 ** float(rng.integers(-3, 4))).astype(np.float32)
        if case % 4 == 0:                                          # exact ties: equal columns, the first maximum wins
            a, b = sorted(rng.choice(Cn, 2, replace=False).tolist())
            p[:, a] = np.abs(p).max() + 1; p[:, b] = p[:, a]
            assert evalstep.vote(p) == a
        if case % 7 == 0:
            p = np.round(p)                                        # many ties of small integers
        assert evalstep.vote(p) == int(np.argmax(np.mean(p, axis=0))), case
    assert evalstep.vote(np.zeros((3, 24), np.float32)) == 0


def _refusals(lib):
    """(entry, argument order, good arguments, [(key, bad value, word of the message)])."""
    vp = C.c_void_p
    st = (C.c_int32 * 32)(*range(32))
    neg = (C.c_int32 * 32)(*([0] * 31 + [-1]))
    crop = [("F", 0, b"outside"), ("h0", 5, b"outside"), ("w0", 5, b"outside"), ("h0", -1, b"outside"), ("w0", -1, b"outside"), ("S", 0, b"outside"),
            ("S", 13, b"outside"), ("H", 9, b"outside"), ("W", 9, b"outside")]
    flags = (lib.pc_truth_frame_flags, ("truth", "F", "H", "W", "h0", "w0", "S", "flags"),
             dict(truth=vp(64), F=4, H=12, W=12, h0=2, w0=2, S=8, flags=vp(64)),
             [("truth", None, b"null"), ("flags", None, b"null")] + crop)
    clips = (lib.pc_eval_clips_from_u8, ("video", "truth", "F", "H", "W", "h0", "w0", "S", "starts", "n", "f_skip", "data", "gt"),
             dict(video=vp(64), truth=vp(64), F=20, H=12, W=12, h0=2, w0=2, S=8, starts=st, n=2, f_skip=2, data=vp(64), gt=vp(128)),
             [(k, None, b"null") for k in ("video", "truth", "starts", "data", "gt")] + crop +
             [("n", 0, b"clips outside"), ("n", 33, b"clips outside"), ("n", -1, b"clips outside"), ("f_skip", 0, b"f_skip"), ("f_skip", -2, b"f_skip"),
              ("data", vp(68), b"16-byte"), ("gt", vp(72), b"16-byte"), ("starts", neg, b"negative")])
    vote = (lib.pc_video_vote, ("pred", "n", "C", "label", "n_correct"), dict(pred=vp(64), n=3, C=24, label=1, n_correct=vp(64)),
            [("pred", None, b"null"), ("n_correct", None, b"null"), ("n", 0, b"n = 0"), ("n", -1, b"n = -1"), ("C", 0, b"C = 0"), ("label", -1, b"label"),
             ("label", 24, b"label")])
    return flags, clips, vote


def test_bad_arguments_are_refused_without_gpu(built):
    for fn, order, ok, bad in _refusals(built):
        for key, val, word in bad:
            args = dict(ok, **{key: val})
            if key == "starts" and val is not None:
                args["n"] = 32                                   # the negative start is the last of 32
            rc = fn(*[args[k] for k in order], None)
            assert rc == -1, (fn.__name__, key, val, rc)         # PC_E_ARG, before any HIP call (there is no device here to make one on)
            assert word in built.pc_last_error(), (fn.__name__, key, val, built.pc_last_error())
    assert capi.ABI_VERSION == built.pc_version() >= 106


def test_host_side_of_the_eval_entries_under_asan_ubsan():
    """Every refusal path of the three entries as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/evalclips_host_driver.cpp."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/evalclips_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "evalclips_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_synthetic_u8_videos():
    hw = 32
    vids = synthetic.make_eval_videos_u8(4, seed=5, num_classes=21, hw=hw, frames_hw=(40, 56))
    again = synthetic.make_eval_videos_u8(4, seed=5, num_classes=21, hw=hw, frames_hw=(40, 56))
    assert len(vids) == 4
    h0, w0 = evalstep.centre_crop(40, 56, hw)
    assert (h0, w0) == (4, 12)
    for vi, ((frames, truth, label), (f2, t2, l2)) in enumerate(zip(vids, again)):
        F = frames.shape[0]
        assert 8 <= F <= 40 and frames.dtype == np.uint8 and frames.shape == (F, 40, 56, 3)
        assert truth.dtype == np.uint8 and truth.shape == (F, 40, 56, 1) and set(np.unique(truth).tolist()) == {0, 1}
        assert label == vi % 21 and np.array_equal(frames, f2) and np.array_equal(truth, t2) and label == l2
        inside = np.count_nonzero(truth[:, h0:h0 + hw, w0:w0 + hw].reshape(F, -1), axis=1)
        if vi == 1:                                                # the box lies wholly outside the centre crop: the video is skipped
            assert truth.sum() > 0 and inside.sum() == 0 and evalstep.clip_starts(F, inside) == []
        else:
            assert evalstep.clip_starts(F, inside)
    default = synthetic.make_eval_videos_u8(1, hw=hw)[0][0]
    assert default.shape[1:] == (hw + 16, hw + 32, 3)              # larger than the crop by default
    with pytest.raises(ValueError):
        synthetic.make_eval_videos_u8(1, hw=hw, frames_hw=(hw, hw + 8))


def test_eval_plan_is_the_forward_list_alone():
    """EvalEngine's plan: one plan of bs clips, the forward list only, and nothing in `prep` / `prep_late` reads what a batch brings (they run
    once per begin())."""
    from types import SimpleNamespace
    p = evalstep.EvalEngine._plan(SimpleNamespace(C=24, hw=72), 3)
    assert len(p.op_to_ndhwc) == 1 and p.lists["fwd"][p.op_to_ndhwc[0]][0] == capi.OP_TO_NDHWC
    assert not any(op[0] == capi.OP_VAL_METRICS for op in p.lists["fwd"])
    per_batch = {p.in_data, p.in_aug, p.in_cls, p.in_labeled, p.img.ref}
    assert not any(r in per_batch for lst in ("prep", "prep_late") for op in p.lists[lst] for r in op[3] if r is not None)
    assert p.img.ref[1] % 16 == 0 and p.out.ref[1] % 16 == 0
