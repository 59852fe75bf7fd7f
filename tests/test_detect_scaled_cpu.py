"""CPU: what detection on a working frame decides on the host, without a GPU.  pc_resample_tables word for word against the numpy
restatement (tests/resample_ref.py) and that restatement's vectorised index against its own Python-integer statement; the identity at equal
sizes; the cap protocol; pc_detect_frames_scaled_ws_bytes; every refusal of pc_detect_frames_scaled before any HIP call -- through capi, and
as a stand-alone program under ASan + UBSan; header, binding and library at ABI 107; the pinned constructor tails; the ValueErrors of
DetectEngine.set_working_frame, which touches no device."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect
from tests import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [(1, 1), (1, 5), (5, 1), (4, 4), (8, 5), (5, 8), (256, 240), (256, 1080), (3, 2 ** 23 - 1)]      # (L, D)


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _library_table(lib, Hs, Ws, H, W):
    n = lib.pc_resample_tables(Hs, Ws, H, W, None, 0)
    assert n == 2 * (H + W)
    tab = np.full(n + 2, 7, np.int32)
    assert lib.pc_resample_tables(Hs, Ws, H, W, C.c_void_p(tab.ctypes.data + 4), n) == n
    assert tab[0] == 7 and tab[-1] == 7
    return tab[1:-1]


@pytest.mark.parametrize("L,D", AXES)
def test_the_vectorised_index_is_the_python_integer_one(L, D):
    i0, w1 = ref.axis_table(L, D)
    ds = range(D) if D <= 2048 else sorted({0, 1, 2, D // 3, D // 2, D - 3, D - 2, D - 1} | set(np.random.default_rng(5).integers(0, D, 4096).tolist()))
    for d in ds:
        a, r, den = ref.axis_pair(L, D, d)
        assert i0[d] == a and w1[d] == np.float32(r) / np.float32(den), (L, D, d)
        assert 0 <= a <= L - 1 and (r == 0 or a < L - 1)                  # a second tap with weight lies inside the source


@pytest.mark.parametrize("L,D", AXES)
def test_resample_tables_equal_the_restatement_word_for_word(built, L, D):
    # as the row axis (beside a one-pixel column axis) and as the column axis: the word after the rows is where the columns start
    got = _library_table(built, L, 1, D, 1)
    assert np.array_equal(got, ref.tables(L, 1, D, 1))
    if D <= 2048:
        got = _library_table(built, 3, L, 2, D)
        assert np.array_equal(got, ref.tables(3, L, 2, D))
    if L == D:                                                          # the identity: every first tap its own index, every weight +0.0
        t = _library_table(built, L, L, D, D)
        assert np.array_equal(t[0::2], np.tile(np.arange(D), 2)) and not t[1::2].any()


def test_the_identity_and_known_answers(built):
    t = _library_table(built, 4, 4, 4, 4)
    assert np.array_equal(t[0::2], np.tile(np.arange(4), 2)) and not t[1::2].any()
    # 2 -> 4: centres at -0.25, 0.25, 0.75, 1.25: clamped, (0, .25), (0, .75), clamped
    i0, w1 = ref.axis_table(2, 4)
    assert i0.tolist() == [0, 0, 0, 1] and w1.tolist() == [0.0, 0.25, 0.75, 0.0]
    # 4 -> 2: centres at 0.5 and 2.5
    i0, w1 = ref.axis_table(4, 2)
    assert i0.tolist() == [0, 2] and w1.tolist() == [0.5, 0.5]
    v, cov = ref.resample(np.arange(16, dtype=np.float32).reshape(4, 4), np.ones((4, 4), np.int32), 2, 2)
    assert v.tolist() == [[2.5, 4.5], [10.5, 12.5]] and cov.all()
    # a NaN or an uncovered pixel under a zero weight poisons nothing; under a non-zero one it does
    M = np.array([[1.0, np.nan], [-0.0, 3.0]], np.float32)
    v, cov = ref.resample(M, np.array([[1, 0], [1, 1]]), 2, 2)
    assert np.array_equal(v.view(np.int32), M.view(np.int32)) and cov.tolist() == [[True, False], [True, True]]
    v, cov = ref.resample(M, np.array([[1, 0], [1, 1]]), 2, 4)
    assert v[0, 0] == 1.0 and np.isnan(v[0, 1:]).all() and cov[0].tolist() == [True, False, False, False] and cov[1].all()
    assert np.signbit(v[1, 0]) and v[1, 1] == np.float32(0.75) and v[1, 3] == 3.0


def test_the_cap_protocol_and_the_refused_sizes(built):
    f = built.pc_resample_tables
    small = np.full(16, 7, np.int32)
    assert f(8, 8, 5, 3, C.c_void_p(small.ctypes.data), 15) == 16 and (small == 7).all()      # too small: the count, nothing written
    assert f(8, 8, 5, 3, None, 1 << 20) == 16                                              # no table: the count
    assert f(8, 8, 5, 3, C.c_void_p(small.ctypes.data), 16) == 16 and np.array_equal(small, ref.tables(8, 8, 5, 3))
    for bad in ((0, 8, 5, 3), (8, 0, 5, 3), (8, 8, 0, 3), (8, 8, 5, 0), (-1, 8, 5, 3), (8, 8, 1 << 23, 3), (8, 8, 5, 1 << 23), (8, 8, 2 ** 31 - 1, 1)):
        assert f(*bad, None, 0) == -1 and b"pc_resample_tables" in built.pc_last_error(), bad
    assert f(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 23 - 1, 2 ** 23 - 1, None, 0) == 4 * (2 ** 23 - 1)    # the largest the library takes


def test_ws_bytes_of_the_scaled_entry(built):
    ws, views_ws = built.pc_detect_frames_scaled_ws_bytes, built.pc_detect_frames_views_ws_bytes
    bad = ((0, 8, 8, 8, 8), (33, 8, 8, 8, 8), (-1, 8, 8, 8, 8), (2, 0, 8, 8, 8), (2, 8, 0, 8, 8), (2, 8, 8, 0, 8), (2, 8, 8, 8, -2),
           (2, 1 << 16, 1 << 15, 8, 8), (2, 8, 8, 1 << 16, 1 << 15), (2, 8, 8, 1 << 23, 1), (2, 8, 8, 1, 1 << 23), (2,) + (2 ** 31 - 1,) * 4)
    assert [ws(*a) for a in bad] == [-1] * len(bad)
    # the partials of a traversal of the NATIVE frame, 16 bytes to align the plane, a float and a cover byte per working pixel of n * 8 frames
    for n, Hs, Ws, H, W in ((1, 3, 3, 9, 11), (2, 8, 12, 8, 12), (8, 120, 136, 90, 160), (32, 256, 256, 240, 320), (1, 256, 256, 1080, 1920), (3, 5, 7, 1, 1)):
        assert ws(n, Hs, Ws, H, W) == views_ws(n, H, W) + 16 + n * 8 * ((Hs * Ws + 3) // 4 * 4) * 5, (n, Hs, Ws, H, W)
    assert ws(32, 256, 256, 240, 320) == 32 * 8 * 19 * 32 + 16 + 83886080                   # 84 MB of plane at n = 32


def _refusals():
    vp = C.c_void_p
    st = (C.c_int32 * 32)(*range(32))
    neg = (C.c_int32 * 32)(*([0] * 31 + [-1]))
    good = [(v % 5, v % 4, v & 1) for v in range(32)]

    def table(last):
        return (C.c_int32 * 96)(*[x for r in good[:31] + [last] for x in r])

    order = ("logits", "F", "H", "W", "Hs", "Ws", "S", "views", "V", "view_stride", "starts", "n", "f_skip", "row0", "dev_tab", "mask", "prob", "rec", "ws")
    ok = dict(logits=vp(64), F=20, H=9, W=10, Hs=12, Ws=12, S=8, views=table((4, 4, 1)), V=2, view_stride=2, starts=st, n=2, f_skip=2, row0=0,
              dev_tab=vp(64), mask=vp(64), prob=vp(64), rec=vp(64), ws=vp(64))
    bad = [(k, None, b"null") for k in ("logits", "views", "starts", "rec", "ws", "dev_tab")] + \
          [("F", 0, b"outside"), ("S", 0, b"outside"), ("S", 16, b"outside"), ("Hs", 7, b"outside"), ("Ws", 7, b"outside")] + \
          [("views", table(last), b"outside") for last in ((5, 2, 0), (2, 5, 0), (-1, 2, 0), (2, -1, 1), (2 ** 31 - 5, 0, 0), (0, 2 ** 31 - 1, 1))] + \
          [("views", table((4, 4, fl)), b"flip") for fl in (2, -1, 256)] + \
          [("V", 0, b"views outside"), ("V", 33, b"views outside"), ("V", -1, b"views outside"), ("view_stride", 1, b"view_stride"),
           ("view_stride", 0, b"view_stride"), ("n", 0, b"clips outside"), ("n", 33, b"clips outside"), ("f_skip", 0, b"f_skip"),
           ("starts", neg, b"negative"), ("S", 6, b"multiple of 4"), ("logits", vp(68), b"16-byte"), ("ws", vp(68), b"aligned"),
           ("rec", vp(66), b"aligned"), ("row0", -1, b"row0"), ("row0", 2 ** 31 - 1000, b"row0")] + \
          [("H", 0, b"native"), ("W", 0, b"native"), ("H", -4, b"native"), ("H", 1 << 23, b"2^24"), ("W", 1 << 23, b"2^24"), ("prob", vp(65), b"2-byte")]
    return order, ok, bad


def test_bad_arguments_are_refused_without_gpu(built):
    order, ok, bad = _refusals()
    fn = built.pc_detect_frames_scaled
    for key, val, word in bad:
        args = dict(ok, **{key: val})
        if key == "starts" and val is not None:
            args["n"] = args["view_stride"] = 32             # the negative start is the last of 32
        if key == "views" and val is not None:
            args["V"] = 32                                   # the bad view is the last of 32
        rc = fn(*[args[k] for k in order], None)
        assert rc == -1, (key, val, rc)                      # PC_E_ARG, before any HIP call (there is no device here to make one on)
        assert word in built.pc_last_error() and b"pc_detect_frames_scaled" in built.pc_last_error(), (key, val, built.pc_last_error())
    for H, W, Hs, Ws in ((1 << 16, 1 << 15, 12, 12), (9, 10, 1 << 16, 1 << 16)):                  # either frame of 2^31 pixels
        rc = fn(*[dict(ok, H=H, W=W, Hs=Hs, Ws=Ws)[k] for k in order], None)
        assert rc == -1 and b"2^31" in built.pc_last_error()


def test_header_binding_and_library_agree_on_the_scaled_entries_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_resample_tables", "pc_detect_frames_scaled_ws_bytes", "pc_detect_frames_scaled"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header), name
        getattr(built, name)


def test_host_side_of_the_scaled_entries_under_asan_ubsan():
    """The table builder into arrays of exactly its size and every refusal path of the launch entry as a stand-alone program against the
    sanitizer build of the library (no GPU, nothing loaded into Python): tests/detect_scaled_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/detect_scaled_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "detect_scaled_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_constructor_tails_stay_and_the_feature_is_a_method_and_attributes():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"
    assert list(inspect.signature(detect.DetectEngine.set_working_frame).parameters) == ["self", "size", "interpolation"]
    assert detect.Detection.work is None
    d = detect.Detection(3, 0.5, np.zeros(24, np.float32), np.zeros(2, np.int32), np.zeros((2, 4), np.int32), np.zeros(2, np.float32), None)
    assert d.work is None and "work" not in vars(d)
    assert detect.INTERPOLATIONS == {"nearest": 0, "linear": 1, "area": 3}


def test_set_working_frame_refuses_what_it_cannot_take():
    de = detect.DetectEngine.__new__(detect.DetectEngine)               # the method reads hw and writes work: no device
    de.hw, de.work = 112, None
    de.set_working_frame((120, 136))
    assert de.work == (120, 136, "area") and de._frame(90, 160) == (120, 136)
    de.set_working_frame([112, np.int64(200)], "nearest")
    assert de.work == (112, 200, "nearest")
    for size, interp in (((111, 136), "area"), ((120, 100), "area"), ((120,), "area"), ((120, 136, 3), "area"), (120, "area"), ((120.0, 136), "area"),
                         (("120", 136), "area"), ((True, 136), "area"), ((None, 136), "area"), ((120, 136), "cubic"), ((120, 136), 3), ((120, 136), None),
                         ((1 << 16, 1 << 15), "area")):
        with pytest.raises(ValueError, match="set_working_frame"):
            de.set_working_frame(size, interp)
        assert de.work == (112, 200, "nearest")                         # a refusal changes nothing
    de.set_working_frame(None)
    assert de.work is None and de._frame(90, 160) == (90, 160)
    de.set_working_frame(size=(256, 256), interpolation="linear")
    assert de.work == (256, 256, "linear")
