"""CPU: what cutting a pass at a chosen mask threshold decides on the host, without a GPU.  detect.cut_word is the sweep's word for the same
float and inverts w / 65535 for every word; the refusals of pc_prob_cut before any HIP call -- through capi, and as a stand-alone program
under ASan + UBSan --, pc_prob_cut_ws_bytes, the numpy restatement against the definition, the names and constructors the feature must not
touch, the signatures of set_mask_threshold / recut, and the setter's refusals."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, ops

from tests import prob_cut_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = C.c_void_p
ORDER = ("prob", "F", "H", "W", "f0", "nf", "word", "mask", "rec", "ws")
OK = dict(prob=vp(66), F=4, H=12, W=12, f0=0, nf=4, word=32768, mask=vp(1027), rec=vp(2048), ws=vp(4096))
# (argument, value, a word of the message)
BAD = [("prob", None, b"null"), ("rec", None, b"null"), ("ws", None, b"null"),
       ("F", 0, b"outside"), ("F", -2, b"outside"), ("H", 0, b"outside"), ("H", -1, b"outside"), ("W", 0, b"outside"), ("W", -3, b"outside"),
       ("f0", -1, b"f0"), ("nf", 0, b"f0"), ("nf", -1, b"f0"), ("nf", 5, b"f0"), ("f0", 1, b"f0"), ("f0", 4, b"f0"), ("f0", 2 ** 31 - 1, b"f0"),
       ("word", 0, b"word ="), ("word", -1, b"word ="), ("word", 65536, b"word ="), ("word", 2 ** 31 - 1, b"word ="), ("word", -2 ** 31, b"word ="),
       ("prob", vp(67), b"prob must be"), ("rec", vp(2049), b"rec must be"), ("rec", vp(2050), b"rec must be"), ("rec", vp(2051), b"rec must be"),
       ("ws", vp(4097), b"ws must be"), ("ws", vp(4098), b"ws must be"), ("ws", vp(4100), b"ws must be"), ("ws", vp(4103), b"ws must be")]
SIZE_BAD = [(1 << 16, 1 << 15), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 2), (46341, 46341)]          # H * W >= 2^31
THRESHOLDS_BAD = (0.0, -0.1, 1.0 + 1e-12, 2, float("nan"), float("inf"), [], [0.5], [[0.5]], (0.2, 0.4), "a", None, np.array([0.5, 0.6]))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def _refused(lib, args, word):
    rc = lib.pc_prob_cut(*[args[k] for k in ORDER], None)
    assert rc == -1, (args, rc)                              # PC_E_ARG, before any HIP call (there is no device here to make one on)
    msg = lib.pc_last_error()
    assert word in msg and b"pc_prob_cut" in msg, (word, msg)


# ---------------------------------------------------------------------- the word
def test_cut_word_is_the_sweeps_word():
    assert detect.cut_word(0.5) == 32768 and detect.cut_word(1.0) == 65535 and detect.cut_word(1.0 / 65535.0) == 1
    assert type(detect.cut_word(0.5)) is int
    assert detect.cut_word(1e-9) == 1 and detect.cut_word(0.50001) == 32769 and detect.cut_word(np.float32(0.25)) == 16384
    for t in detect.DEFAULT_SWEEP:
        assert detect.cut_word(t) == int(detect.threshold_words([t])[0])
    assert [detect.cut_word(t) for t in detect.DEFAULT_SWEEP] == detect.threshold_words().tolist()
    for bad in THRESHOLDS_BAD:
        with pytest.raises(ValueError, match="threshold_words"):
            detect.cut_word(bad)


def test_every_word_round_trips_through_its_threshold():
    """A word read off a SweepScore can be handed back as a threshold exactly: cut_word(w / 65535) == w for all 65535 of them."""
    w = np.arange(1, 65536, dtype=np.int64)
    t = w.astype(np.float64) / 65535.0
    assert np.array_equal(np.ceil(t * 65535.0).astype(np.int64), w)          # the rule cut_word applies, on all words at once
    for k in range(1, 65536):
        assert detect.cut_word(k / 65535) == k


# ---------------------------------------------------------------------- the entries
def test_prob_cut_refuses_bad_arguments_without_gpu(built):
    for key, val, word in BAD:
        _refused(built, dict(OK, **{key: val}), word)
    for H, W in SIZE_BAD:
        _refused(built, dict(OK, H=H, W=W), b"2^31")
    _refused(built, dict(OK, F=2 ** 31 - 1, f0=2 ** 31 - 1, nf=2 ** 31 - 1), b"f0")          # f0 + nf beyond int32
    _refused(built, dict(OK, mask=None, word=0), b"word =")                                  # a null mask is no refusal; the word is


def test_ws_bytes_is_host_arithmetic_and_minus_one_where_the_call_refuses(built):
    ws = built.pc_prob_cut_ws_bytes
    assert ws(1, 1, 1) == 32                                 # one block, one partial of 32 bytes
    assert ws(3, 5, 7) == 3 * 32
    assert ws(1, 64, 64) == 32 and ws(1, 64, 65) == 2 * 32   # 1024 groups of four: the last that one block takes
    assert ws(5, 120, 136) == 5 * 4 * 32
    assert ws(40, 240, 320) == 40 * 19 * 32                  # 19200 groups of four at 1024 a block
    assert ws(1, 1080, 1920) == 64 * 32                      # the cap of 64 blocks per frame
    assert ws(1, 1, 256 * 1024) == 64 * 32 and ws(1, 1, 63 * 4096) == 63 * 32
    assert ws(2 ** 31 - 1, 46340, 46340) == (2 ** 31 - 1) * 64 * 32           # the largest of all: no overflow in int64
    assert ops.prob_cut_ws_bytes(40, 240, 320) == ws(40, 240, 320)
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, -4), (1, 1 << 16, 1 << 15), (1, 2 ** 31 - 1, 2 ** 31 - 1), (1, 46341, 46341)):
        assert ws(*bad) == -1, bad
        with pytest.raises(ValueError, match="prob_cut_ws_bytes"):
            ops.prob_cut_ws_bytes(*bad)


def test_host_side_of_the_entries_under_asan_ubsan():
    """Every refusal path and the workspace arithmetic as a stand-alone program against the sanitizer build of the library (no GPU, nothing
    loaded into Python): tests/prob_cut_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/prob_cut_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "prob_cut_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_header_binding_and_library_agree_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_prob_cut", "pc_prob_cut_ws_bytes"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header)
        getattr(built, name)
    assert int(re.search(r"#define\s+PC_PROB_ONE\s+(\d+)", header).group(1)) == ops.PROB_ONE == ref.ONE == 65535
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^asan:.*\bprob_cut\b", mk, re.M) and re.search(r"^SRCS\s*=.*\bprobcut\.hip\b", mk, re.M)
    assert re.search(r"^HDRS\s*=.*\bprobwords\.h\b", mk, re.M)
    # the group loader is said once, in the header both translation units include
    for unit in ("probhist.hip", "probcut.hip"):
        with open(os.path.join(csrc, unit)) as f:
            text = f.read()
        assert '#include "probwords.h"' in text and not re.search(r"uint2\s+prob_words\s*\(", text), unit


# ---------------------------------------------------------------------- the restatement against the definition
def test_restatement_on_maps_with_known_answers():
    p = np.zeros((3, 4, 6), np.uint16)
    p[0, 1, 2], p[0, 3, 5], p[0, 2, 0] = 40000, 50000, 39999
    p[2] = 65535
    m, r = ref.cut(p, 40000)
    assert m.dtype == np.uint8 and m.sum() == 2 + 24 and m[0, 1, 2] == m[0, 3, 5] == 1 and m[0, 2, 0] == 0
    assert r.dtype == np.int32 and r.shape == (3, 6)
    assert r[0, :5].tolist() == [2, 2, 1, 6, 4] and r[0, 5:].view(np.float32)[0] == np.float32(90000.0 / (65535.0 * 2))
    assert not r[1].any()
    assert r[2, :5].tolist() == [24, 0, 0, 6, 4] and r[2, 5:].view(np.float32)[0] == np.float32(1.0)
    assert not ref.cut(p, 65535)[1][0].any() and ref.cut(p, 1)[1][0, 0] == 3


# ---------------------------------------------------------------------- names, constructors, signatures
def test_constructors_keep_their_last_parameters_and_the_new_methods_their_signatures():
    assert list(inspect.signature(detect.DetectEngine.__init__).parameters)[-1] == "instance_links"
    assert list(inspect.signature(detect.Detection.__init__).parameters)[-1] == "inst_overlaps"
    assert detect.Detection.threshold is None and detect.Detection.work is None and detect.Detection.hop is None
    sig = inspect.signature(detect.DetectEngine.set_mask_threshold).parameters
    assert list(sig) == ["self", "threshold"] and sig["threshold"].default is None
    sig = inspect.signature(detect.DetectEngine.recut).parameters
    assert list(sig) == ["self", "threshold", "videos"] and sig["threshold"].default is inspect.Parameter.empty and sig["videos"].default is None
    assert list(inspect.signature(detect.cut_word).parameters) == ["threshold"]
    sig = inspect.signature(ops.prob_cut).parameters
    assert list(sig) == ["prob", "word", "f0", "nf", "mask", "rec", "ws", "want_mask"]
    assert [sig[k].default for k in list(sig)[2:]] == [0, None, None, None, None, True]
    assert list(inspect.signature(ops.prob_cut_ws_bytes).parameters) == ["nf", "H", "W"]
    assert "IN PLACE" in detect.DetectEngine.recut.__doc__


def test_set_mask_threshold_refuses_what_threshold_words_refuses_and_a_bool():
    eng = detect.DetectEngine.__new__(detect.DetectEngine)   # the setter touches one field: no device is needed to see it refuse
    assert eng.mask_threshold is None
    for keep in (None, (0.35, 22938)):
        eng.set_mask_threshold(None if keep is None else keep[0])
        assert eng.mask_threshold == keep
        for bad in THRESHOLDS_BAD + (True, False, np.True_):
            if bad is None:
                continue                                      # None is the way back, not a refusal
            with pytest.raises(ValueError, match="set_mask_threshold"):
                eng.set_mask_threshold(bad)
            assert eng.mask_threshold == keep
    eng.set_mask_threshold(0.5)
    assert eng.mask_threshold == (0.5, 32768) and type(eng.mask_threshold[0]) is float and type(eng.mask_threshold[1]) is int
    eng.set_mask_threshold(np.float32(0.25))
    assert eng.mask_threshold == (0.25, 16384)
    eng.set_mask_threshold(40000 / 65535)
    assert eng.mask_threshold[1] == 40000
    eng.set_mask_threshold()
    assert eng.mask_threshold is None
    assert "mask_threshold" not in detect.DetectEngine.__new__(detect.DetectEngine).__dict__
