"""CPU: what overlapping clips in time decide on the host, without a GPU.  The window rule (csrc/cliphop.h) through pc_clip_hop_starts, against
detect.clip_starts_hop and against a restatement written here, for f_skip 1..3, every legal hop and F = 1..119, with the six properties the
kernels build on: ascending and distinct starts, the clip index, equality with evalstep.clip_starts at the full span, the window count, the
cover range of a frame, pairwise distinct slots.  pc_clip_planes_bytes / pc_detect_frames_planes_ws_bytes; every refusal of pc_clip_planes and
pc_detect_frames_planes before any HIP call -- through capi, and as a stand-alone program under ASan + UBSan; header, binding and library at
ABI 107; the pinned constructor tails; DetectEngine.set_clip_hop, which touches no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, evalstep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [(fs, hop) for fs in (1, 2, 3) for hop in range(fs, 8 * fs + 1, fs)]
FRAMES = range(1, 120)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _ceil(a, b):
    return -(-a // b)


def _restated(F, fs, hop):
    """The rule of the issue, word for word: windows at i = m * hop, kept iff i == 0 or i - hop + span < F; starts i + j, j < fs, i + j < F."""
    span, out, i = 8 * fs, [], 0
    while i == 0 or i - hop + span < F:
        out += [i + j for j in range(fs) if i + j < F]
        i += hop
    return out


def _library(lib, F, fs, hop):
    n = lib.pc_clip_hop_starts(F, fs, hop, None, 0)
    assert n >= 1
    st = np.full(n + 2, -7, np.int32)
    assert lib.pc_clip_hop_starts(F, fs, hop, C.c_void_p(st.ctypes.data + 4), n) == n
    assert st[0] == -7 and st[-1] == -7
    return st[1:-1].tolist()


@pytest.mark.parametrize("fs,hop", RULES)
def test_library_python_and_restatement_give_the_same_starts(built, fs, hop):
    for F in FRAMES:
        want = _restated(F, fs, hop)
        assert _library(built, F, fs, hop) == want, (F, fs, hop)
        assert detect.clip_starts_hop(F, fs, hop) == want, (F, fs, hop)


@pytest.mark.parametrize("fs,hop", RULES)
def test_the_six_properties_of_the_window_rule(fs, hop):
    span, M = 8 * fs, _ceil(8 * fs, hop)
    assert 1 <= M <= 8
    for F in FRAMES:
        st = detect.clip_starts_hop(F, fs, hop)
        # ascending and distinct
        assert all(a < b for a, b in zip(st, st[1:])) and st[0] == 0 and st[-1] < F
        # the clip index
        for i, s in enumerate(st):
            assert s % hop < fs and (s // hop) * fs + s % hop == i, (F, s)
        # equal at full span
        if hop == span:
            assert st == evalstep.clip_starts(F, np.ones(F, np.int32), fs)
        # the window count
        windows = sorted({s // hop for s in st})
        assert windows == list(range(len(windows)))
        assert len(windows) == (1 if F <= span else 1 + _ceil(F - span, hop)), (F, len(windows))
        # cover: the windows whose span holds the frame are lo .. hi, 1..M of them; in each the frame is frame k of the clip of phase f % fs
        for f in range(F):
            holding = [m for m in windows if m * hop <= f < m * hop + span]
            lo, hi = max(0, _ceil(f - span + 1, hop)), min(f // hop, len(windows) - 1)
            assert holding == list(range(lo, hi + 1)) and 1 <= len(holding) <= M, (F, f, holding, lo, hi)
            for m in holding:
                s = m * hop + f % fs
                assert s in st and (f - s) % fs == 0 and 0 <= (f - s) // fs < 8
            # slots
            assert len({m % M for m in holding}) == len(holding)
            # the first clip that holds the frame: what pc_detect_frames_planes writes into record word 6 (times V, plus row0)
            assert st[lo * fs + f % fs] == lo * hop + f % fs


def test_the_cap_protocol_and_the_refused_rules(built):
    f = built.pc_clip_hop_starts
    small = np.full(8, -7, np.int32)
    assert f(40, 2, 8, C.c_void_p(small.ctypes.data), 7) == 8 and (small == -7).all()        # too small: the count, nothing written
    assert f(40, 2, 8, None, 1 << 20) == 8                                                # no array: the count
    assert f(40, 2, 8, C.c_void_p(small.ctypes.data), 8) == 8 and small.tolist() == [0, 1, 8, 9, 16, 17, 24, 25]
    assert f(17, 2, 8, None, 0) == 4 and f(17, 2, 16, None, 0) == 3 and f(16, 2, 8, None, 0) == 2 and f(1, 3, 3, None, 0) == 1
    for bad in ((0, 2, 8), (-1, 2, 8), (17, 0, 8), (17, -2, 8), (17, 2, 0), (17, 2, 1), (17, 2, 3), (17, 2, 18), (17, 3, 4), (17, (1 << 20) + 1, (1 << 20) + 1)):
        assert f(*bad, None, 0) == -1 and b"pc_clip_hop_starts" in built.pc_last_error(), bad
        if bad[0] >= 1:
            with pytest.raises(ValueError, match="clip_starts_hop"):
                detect.clip_starts_hop(*bad)
    with pytest.raises(ValueError, match="clip_starts_hop"):
        detect.clip_starts_hop(0, 2, 8)


def test_bytes_of_the_planes_and_of_the_partials(built):
    pb, wb = built.pc_clip_planes_bytes, built.pc_detect_frames_planes_ws_bytes
    bad = ((0, 8, 8, 2, 8), (17, 0, 8, 2, 8), (17, 8, -1, 2, 8), (17, 1 << 16, 1 << 15, 2, 8), (17, 8, 8, 2, 7), (17, 8, 8, 0, 0), (17, 8, 8, 2, 18),
           (2 ** 31 - 1, 46340, 46340, 1, 1))
    assert [pb(*a) for a in bad] == [-1] * len(bad)
    for F, Hs, Ws, fs, hop in ((17, 3, 3, 2, 8), (40, 10, 12, 2, 6), (40, 10, 12, 2, 2), (40, 10, 13, 2, 4), (33, 12, 16, 2, 8), (20, 10, 12, 3, 3), (5, 256, 256, 2, 16)):
        ps, M = (Hs * Ws + 3) // 4 * 4, _ceil(8 * fs, hop)
        assert pb(F, Hs, Ws, fs, hop) == M * F * ps * 4 + ps, (F, Hs, Ws, fs, hop)
    assert [wb(*a) for a in ((0, 8, 8), (257, 8, 8), (1, 0, 8), (1, 8, -3), (1, 1 << 16, 1 << 15))] == [-1] * 5
    assert wb(1, 9, 11) == 32 and wb(256, 240, 320) == 256 * 19 * 32 and wb(3, 1080, 1920) == 3 * 64 * 32
    assert wb(7, 120, 136) == 7 * built.pc_detect_frames_views_ws_bytes(1, 120, 136) // 8       # the partials of the views traversal, per frame


def _views_table(last):
    good = [(v % 5, v % 4, v & 1) for v in range(32)]
    return (C.c_int32 * 96)(*[x for r in good[:31] + [last] for x in r])


def test_clip_planes_refuses_bad_arguments_without_gpu(built):
    vp = C.c_void_p
    st = (C.c_int32 * 32)(*[(c // 2) * 8 + c % 2 for c in range(32)])

    def table(*vals):
        return (C.c_int32 * 32)(*(list(st[:32 - len(vals)]) + list(vals)))

    order = ("logits", "F", "Hs", "Ws", "S", "views", "V", "view_stride", "starts", "n", "f_skip", "hop", "plane", "cover")
    ok = dict(logits=vp(64), F=400, Hs=12, Ws=12, S=8, views=_views_table((4, 4, 1)), V=2, view_stride=2, starts=st, n=2, f_skip=2, hop=8, plane=vp(64), cover=vp(64))
    bad = [(k, None, b"null") for k in ("logits", "views", "starts", "plane")] + \
          [("F", 0, b"outside"), ("S", 0, b"outside"), ("S", 16, b"outside"), ("Hs", 7, b"outside"), ("Ws", 7, b"outside"), ("S", 6, b"multiple of 4")] + \
          [("views", _views_table(last), b"outside") for last in ((5, 2, 0), (2, 5, 0), (-1, 2, 0), (2, -1, 1), (2 ** 31 - 5, 0, 0), (0, 2 ** 31 - 1, 1))] + \
          [("views", _views_table((4, 4, fl)), b"flip") for fl in (2, -1, 256)] + \
          [("V", 0, b"views outside"), ("V", 33, b"views outside"), ("view_stride", 1, b"view_stride"), ("n", 0, b"clips outside"), ("n", 33, b"clips outside"),
           ("f_skip", 0, b"f_skip")] + [("hop", h, b"hop") for h in (0, 1, 7, 18, 32, -8, 2 ** 31 - 1)] + \
          [("starts", table(-1), b"negative"), ("starts", table(122), b"no clip start"), ("starts", table(49 * 8), b"no clip start"),      # window 49 of 400 frames is not kept: window 48 reaches the end
           ("logits", vp(68), b"16-byte"), ("plane", vp(72), b"16-byte"), ("cover", vp(66), b"4-byte")]
    fn = built.pc_clip_planes
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        if key == "starts" and val is not None:
            args["n"] = args["view_stride"] = 32             # the bad start is the last of 32
        if key == "views" and val is not None:
            args["V"] = 32                                   # the bad view is the last of 32
        rc = fn(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                      # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error() and b"pc_clip_planes" in built.pc_last_error(), (key, val, built.pc_last_error())
    # a cover with a first clip that holds no frame; a frame of 2^31 pixels
    first_past = (C.c_int32 * 32)(*([400] + list(st[1:])))
    assert fn(*[dict(ok, starts=first_past)[k] for k in order], None) == -1 and b"cover" in built.pc_last_error()
    assert fn(*[dict(ok, Hs=1 << 16, Ws=1 << 16)[k] for k in order], None) == -1 and b"2^31" in built.pc_last_error()


def test_detect_frames_planes_refuses_bad_arguments_without_gpu(built):
    vp = C.c_void_p
    order = ("plane", "cover", "F", "H", "W", "Hs", "Ws", "V", "f_skip", "hop", "f0", "nf", "row0", "dev_tab", "mask", "prob", "rec", "ws")
    ok = dict(plane=vp(64), cover=vp(64), F=40, H=9, W=10, Hs=12, Ws=12, V=2, f_skip=2, hop=8, f0=0, nf=40, row0=0, dev_tab=vp(64), mask=vp(64), prob=vp(64),
              rec=vp(64), ws=vp(64))
    bad = [(k, None, b"null") for k in ("plane", "cover", "dev_tab", "rec", "ws")] + \
          [("F", 0, b"F = 0"), ("H", 0, b"native"), ("W", -3, b"native"), ("Hs", 0, b"working"), ("Ws", -(2 ** 31), b"working"), ("H", 1 << 23, b"2^24"),
           ("W", 1 << 23, b"2^24"), ("V", 0, b"views outside"), ("V", 33, b"views outside"), ("f_skip", 0, b"hop")] + \
          [("hop", h, b"hop") for h in (0, 1, 7, 18, 32, -8, 2 ** 31 - 1)] + \
          [("f0", -1, b"outside the video"), ("nf", 0, b"outside the video"), ("nf", 41, b"outside the video"), ("f0", 1, b"outside the video"),
           ("nf", 2 ** 31 - 1, b"outside the video"), ("row0", -1, b"row0"), ("row0", 2 ** 31 - 16, b"row0"),
           ("plane", vp(68), b"aligned"), ("cover", vp(65), b"aligned"), ("dev_tab", vp(66), b"aligned"), ("rec", vp(66), b"aligned"), ("ws", vp(68), b"aligned"),
           ("prob", vp(65), b"2-byte")]
    fn = built.pc_detect_frames_planes
    for key, val, word in bad:
        rc = fn(*[dict(ok, **{key: val})[k] for k in order], None)
        assert rc == -1, (key, val, rc)
        assert word in built.pc_last_error() and b"pc_detect_frames_planes" in built.pc_last_error(), (key, val, built.pc_last_error())
    for H, W, Hs, Ws in ((1 << 16, 1 << 15, 12, 12), (9, 10, 1 << 16, 1 << 16)):                  # either frame of 2^31 pixels
        assert fn(*[dict(ok, H=H, W=W, Hs=Hs, Ws=Ws)[k] for k in order], None) == -1 and b"2^31" in built.pc_last_error()
    assert fn(*[dict(ok, F=400, nf=257)[k] for k in order], None) == -1 and b"outside the video" in built.pc_last_error()      # a range holds 256 frames


def test_header_binding_and_library_agree_on_the_hop_entries_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    assert int(re.search(r"#define\s+PC_PLANES_MAX_FRAMES\s+(\d+)", header).group(1)) == 256
    for name in ("pc_clip_hop_starts", "pc_clip_planes_bytes", "pc_clip_planes", "pc_detect_frames_planes_ws_bytes", "pc_detect_frames_planes"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header), name
        getattr(built, name)


def test_host_side_of_the_hop_entries_under_asan_ubsan():
    """The starts entry into arrays of exactly its size and every refusal path of the two launch entries as a stand-alone program against
    the sanitizer build of the library (no GPU, nothing loaded into Python): tests/clip_hop_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/clip_hop_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "clip_hop_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_constructor_tails_stay_and_the_feature_is_a_method_and_attributes():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"
    assert list(inspect.signature(detect.DetectEngine.set_clip_hop).parameters) == ["self", "hop"]
    assert inspect.signature(detect.DetectEngine.set_clip_hop).parameters["hop"].default is None
    assert detect.Detection.hop is None and detect.DetectEngine.hop is None
    d = detect.Detection(3, 0.5, np.zeros(24, np.float32), np.zeros(2, np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.float32), None)
    assert d.hop is None and "hop" not in vars(d)


def test_set_clip_hop_refuses_what_it_cannot_take():
    de = detect.DetectEngine.__new__(detect.DetectEngine)               # the method reads f_skip and writes hop: no device
    de.f_skip = 2
    assert de.hop is None
    de.set_clip_hop(8)
    assert de.hop == 8
    de.set_clip_hop(np.int64(4))
    assert de.hop == 4 and type(de.hop) is int
    for hop in (0, 1, 3, 18, 32, -2, 4.0, "4", True, (4,), [8]):
        with pytest.raises(ValueError, match="set_clip_hop"):
            de.set_clip_hop(hop)
        assert de.hop == 4                                              # a refusal changes nothing
    de.set_clip_hop(16)                                                 # the full span: today's cut
    assert de.hop is None
    de.set_clip_hop(2)
    assert de.hop == 2
    de.set_clip_hop()
    assert de.hop is None
    de.f_skip = 3
    de.set_clip_hop(hop=9)
    assert de.hop == 9
    with pytest.raises(ValueError, match="set_clip_hop"):
        de.set_clip_hop(8)
