"""CPU: what the run-length export decides on the host, without a GPU.  The refusals of pc_mask_run_index / pc_mask_runs before any HIP
call -- through capi, and as a stand-alone program under ASan + UBSan --, pc_mask_run_ws_bytes, the numpy restatement
(tests/mask_runs_ref.py) against ops.decode_mask_runs and detect.MaskRuns, and the constructors the feature must not touch."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, ops

from tests import mask_runs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
INDEX_ORDER = ("map", "F", "H", "W", "f0", "nf", "index", "ws")
RUNS_ORDER = ("map", "F", "H", "W", "f0", "nf", "index", "cap", "runs")
OK = dict(map=vp(65), F=4, H=12, W=12, f0=0, nf=4, index=vp(64), ws=vp(128), cap=C.c_int64(4), runs=vp(256))
# (argument, value, a word of the message) for both entries
RANGE_BAD = [("map", None, b"map is null"), ("index", None, b"index is null"), ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"),
             ("H", -1, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"), ("W", 65536, b"W ="), ("W", 2 ** 31 - 1, b"W ="), ("f0", -1, b"f0"),
             ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
             ("index", vp(66), b"index must be"), ("index", vp(65), b"index must be"), ("index", vp(67), b"index must be")]
# (F = nf, H, W, a word of the message): the row field and the int32 run count
SIZE_BAD = [(4097, 4096, 1, b"2^24"), (2, 2 ** 31 - 1, 1, b"2^24"), (2 ** 31 - 1, 2 ** 31 - 1, 1, b"2^24"), (8, 1 << 14, 1 << 14, b"2^31"),
            (1, 1 << 16, 1 << 15, b"2^31"), (1 << 12, 1 << 12, 65535, b"2^31")]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _refused(lib, entry, order, args, word):
    rc = getattr(lib, entry)(*[args[k] for k in order], None)
    assert rc == -1, (entry, args, rc)                       # PC_E_ARG, before any HIP call (there is no device here to make one on)
    msg = lib.pc_last_error()
    assert word in msg and entry.encode() in msg, (entry, word, msg)


# ---------------------------------------------------------------------- the entries
def test_mask_run_entries_refuse_bad_arguments_without_gpu(built):
    for entry, order in (("pc_mask_run_index", INDEX_ORDER), ("pc_mask_runs", RUNS_ORDER)):
        for key, val, word in RANGE_BAD:
            _refused(built, entry, order, dict(OK, **{key: val}), word)
        for F, H, W, word in SIZE_BAD:
            _refused(built, entry, order, dict(OK, F=F, nf=F, H=H, W=W), word)
    for val in (None,):
        _refused(built, "pc_mask_run_index", INDEX_ORDER, dict(OK, ws=val), b"ws is null")
    for val in (vp(129), vp(130), vp(131)):
        _refused(built, "pc_mask_run_index", INDEX_ORDER, dict(OK, ws=val), b"ws must be")
    for cap in (1, 4, 2 ** 63 - 1):
        _refused(built, "pc_mask_runs", RUNS_ORDER, dict(OK, runs=None, cap=C.c_int64(cap)), b"runs is null")
    for cap in (-1, -2 ** 63):
        _refused(built, "pc_mask_runs", RUNS_ORDER, dict(OK, cap=C.c_int64(cap)), b"cap =")
        _refused(built, "pc_mask_runs", RUNS_ORDER, dict(OK, cap=C.c_int64(cap), runs=None), b"cap =")
    for val in (vp(257), vp(258), vp(259)):
        _refused(built, "pc_mask_runs", RUNS_ORDER, dict(OK, runs=val), b"runs must be")
        _refused(built, "pc_mask_runs", RUNS_ORDER, dict(OK, runs=val, cap=C.c_int64(0)), b"runs must be")


def test_ws_bytes_is_minus_one_where_the_calls_refuse(built):
    ws = built.pc_mask_run_ws_bytes
    assert ws(1, 1) >= 4 and ws(1, 1) % 4 == 0
    assert 4 <= ws(40, 240) <= 4 * 40 * 240 and ws(40, 240) % 4 == 0
    assert ws(1 << 12, 1 << 12) > 0                          # 2^24 rows: the last that fit
    assert ws(4, 12) == ws(12, 4) == ws(1, 48)               # a function of the rows of the range
    for nf, H in ((0, 4), (4, 0), (-1, 4), (4, -1), ((1 << 12) + 1, 1 << 12), (2 ** 31 - 1, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (2 ** 31 - 1, 1)):
        assert ws(nf, H) == -1, (nf, H)
        if nf >= 1 and H >= 1:                               # ... and there the calls refuse the same range
            _refused(built, "pc_mask_run_index", INDEX_ORDER, dict(OK, F=nf, nf=nf, H=H, W=1), b"2^24")


def test_host_side_of_the_entries_under_asan_ubsan():
    """Every refusal path of the three entries as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/mask_runs_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/mask_runs_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "mask_runs_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_mask_run_ws_bytes", "pc_mask_run_index", "pc_mask_runs"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header)
        getattr(built, name)
    words = int(re.search(r"#define\s+PC_RUN_WORDS\s+(\d+)", header).group(1))
    assert words == ops.RUN_WORDS == ref.RUN_WORDS == 2
    with open(os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\bmask_runs\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bmaskruns\.hip\b", mk, re.M)


def test_constructors_keep_their_last_parameters():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"


# ---------------------------------------------------------------------- the format
HAND_ROW = [0, 1, 1, 2, 2, 0, 2, 255]
HAND_RUNS = [(1, 3, 1), (3, 5, 2), (6, 7, 2), (7, 8, 255)]


def test_the_case_counted_by_hand():
    assert ref.row_runs(HAND_ROW) == HAND_RUNS
    m = np.zeros((2, 3, 8), np.uint8)
    m[1, 1] = HAND_ROW                                       # row 4 of the video
    m[0, 2, 7] = 9                                           # row 2: one pixel at the right edge
    index, runs = ref.runs_of(m)
    assert index.tolist() == [0, 0, 0, 1, 1, 5, 5]
    want = [(2 | 9 << 24, 7 | 8 << 16)] + [(4 | v << 24, x0 | x1 << 16) for x0, x1, v in HAND_RUNS]
    assert runs.dtype == np.uint32 and runs.tolist() == [list(w) for w in want]
    mr = detect.MaskRuns.from_dense(m)
    assert mr.shape == (2, 3, 8) and mr.runs.dtype == np.uint32 and mr.runs.tolist() == runs.tolist()
    assert mr.offsets.dtype == np.int64 and mr.offsets.tolist() == [0, 1, 5]
    y, x0, x1, v = mr.frame(1)
    assert (y.tolist(), x0.tolist(), x1.tolist(), v.tolist()) == ([1, 1, 1, 1], [1, 3, 6, 7], [3, 5, 7, 8], [1, 2, 2, 255])
    y, x0, x1, v = mr.frame(0)
    assert (y.tolist(), x0.tolist(), x1.tolist(), v.tolist()) == ([2], [7], [8], [9])
    assert mr.areas().dtype == np.int64 and mr.areas().tolist() == [1, 6]
    assert mr.nbytes == 5 * 8 + 3 * 8
    assert np.array_equal(mr.dense(), m) and np.array_equal(mr.dense(1), m[1]) and np.array_equal(mr.dense(0), m[0])
    assert mr.dense().dtype == np.uint8 and mr.dense(1).shape == (3, 8)
    one = detect.MaskRuns.from_dense(m[1])                   # a single frame [H, W]
    assert one.shape == (1, 3, 8) and one.offsets.tolist() == [0, 4] and np.array_equal(one.dense(0), m[1])
    for bad in (-1, 2):
        with pytest.raises(ValueError):
            mr.frame(bad)
        with pytest.raises(ValueError):
            mr.dense(bad)


def _maps():
    rng = np.random.default_rng(20261020)
    vals = np.array([1, 2, 9, 255], np.uint8)
    out = []
    for density in (0.08, 0.5, 0.97):
        m = vals[rng.integers(0, 4, size=(3, 19, 37))]
        m[rng.random(m.shape) >= density] = 0
        out.append(m)
    blocks = np.repeat(np.repeat(vals[rng.integers(0, 4, size=(2, 5, 6))] * (rng.random((2, 5, 6)) < 0.6), 4, axis=1), 7, axis=2)
    out.append(np.ascontiguousarray(blocks.astype(np.uint8)))               # long runs, touching runs of different values
    out.append(np.zeros((2, 5, 9), np.uint8))
    out.append(np.full((2, 5, 9), 255, np.uint8))
    out.append(np.full((1, 1, 1), 7, np.uint8))
    return out


def test_decoders_invert_the_restatement_and_the_host_encoder():
    for m in _maps():
        nf, H, W = m.shape
        index, runs = ref.runs_of(m)
        assert index[0] == 0 and index[-1] == runs.shape[0] and (np.diff(index) >= 0).all()
        assert np.array_equal(ref.dense_of(runs, nf, H, W), m)
        got = ops.decode_mask_runs(runs, nf, H, W)
        assert got.dtype == np.uint8 and got.shape == m.shape and np.array_equal(got, m)
        assert np.array_equal(ops.decode_mask_runs(runs.view(np.int32), nf, H, W), m)        # the words as the device tensor holds them
        mr = detect.MaskRuns.from_dense(m)
        assert np.array_equal(mr.runs, runs) and np.array_equal(mr.offsets, index[::H].astype(np.int64))
        assert np.array_equal(mr.dense(), m)
        assert np.array_equal(mr.areas(), (m != 0).reshape(nf, -1).sum(axis=1))
        for f in range(nf):
            assert np.array_equal(mr.dense(f), m[f])
    assert ref.runs_of(np.zeros((2, 5, 9), np.uint8))[1].shape == (0, 2)
    assert ref.runs_of(np.full((2, 5, 9), 255, np.uint8))[1].tolist() == [[r | 255 << 24, 9 << 16] for r in range(10)]


def test_decode_and_maskruns_refuse_what_does_not_fit():
    runs = np.array([[1 | 1 << 24, 2 | 5 << 16]], np.uint32)
    assert ops.decode_mask_runs(runs, 1, 2, 5)[0].tolist() == [[0] * 5, [0, 0, 1, 1, 1]]
    for nf, H, W in ((1, 1, 5), (1, 2, 4)):                  # the row, the column outside
        with pytest.raises(ValueError):
            ops.decode_mask_runs(runs, nf, H, W)
    for bad in (np.array([[0 | 1 << 24, 3 | 3 << 16]], np.uint32), np.array([[0, 1 | 2 << 16]], np.uint32), runs.astype(np.int64), runs.reshape(-1)[:1]):
        with pytest.raises(ValueError):                      # empty, value 0, not 32-bit words, half a run
            ops.decode_mask_runs(bad, 1, 2, 5)
    detect.MaskRuns((1, 2, 5), [0, 1], runs)
    for shape, offsets in (((1, 2, 5), [0, 2]), ((1, 2, 5), [1, 1]), ((2, 2, 5), [0, 1]), ((2, 2, 5), [0, 2, 1]), ((1, 2, 65536), [0, 1]), ((0, 2, 5), [0])):
        with pytest.raises(ValueError):
            detect.MaskRuns(shape, offsets, runs)
    for bad in (np.zeros((2, 3), np.int32), np.zeros((2, 2, 2, 2), np.uint8), [[1.0]]):
        with pytest.raises(ValueError):
            detect.MaskRuns.from_dense(bad)


def test_run_ranges_split_a_video_at_the_limits_of_one_call():
    assert detect.run_ranges(40, 240, 320) == [(0, 40)]
    assert detect.run_ranges(2100, 1024, 1024) == [(0, 2047), (2047, 53)]                    # 2047 frames of 2^20 pixels stay below 2^31
    assert detect.run_ranges(5, 1 << 23, 1) == [(0, 2), (2, 2), (4, 1)]                      # the row field: 2^24 rows a range
    for F, H, W in ((2100, 1024, 1024), (70000, 240, 320), (3, 1 << 23, 200)):
        rr = detect.run_ranges(F, H, W)
        assert rr[0][0] == 0 and sum(nf for _f0, nf in rr) == F and all(a[0] + a[1] == b[0] for a, b in zip(rr, rr[1:]))
        assert all(nf * H * W < 2 ** 31 and nf * H <= 2 ** 24 for _f0, nf in rr)
    with pytest.raises(ValueError):
        detect.run_ranges(1, 1 << 16, 1 << 15)
