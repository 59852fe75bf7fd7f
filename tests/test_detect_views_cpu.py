"""CPU: what multi-view detection decides on the host, without a GPU.  detect.make_views (tiling, flips, the cap of 32, explicit views), and the
three C entry points behind DetectEngine(tile=, flip=, views=) -- pc_clips_from_u8_views, pc_detect_frames_views,
pc_detect_frames_views_ws_bytes -- refusing every bad argument before any HIP call: through capi, and as a stand-alone program under
ASan + UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
from picons_amd import capi, detect, evalstep, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(capi.LIB_PATH):
        ge.build()
    return capi.lib()


def test_make_views_tiles_the_frame():
    assert detect.make_views(240, 320, 224, tile=True) == [(0, 0, 0), (0, 96, 0), (16, 0, 0), (16, 96, 0)]
    assert detect.make_views(224, 224, 224, tile=True) == [(0, 0, 0)]
    assert detect.make_views(9, 11, 4, tile=True) == [(h0, w0, 0) for h0 in (0, 2, 5) for w0 in (0, 3, 7)]       # y-major, x-minor
    assert detect.make_views(120, 136, 112, tile=True) == [(0, 0, 0), (0, 24, 0), (8, 0, 0), (8, 24, 0)]
    assert detect.make_views(224, 320, 224, tile=True) == [(0, 0, 0), (0, 96, 0)]


def test_make_views_without_tiling_is_the_centre_crop():
    for H, W, hw in ((240, 320, 224), (120, 136, 112), (9, 11, 4), (224, 224, 224)):
        h0, w0 = evalstep.centre_crop(H, W, hw)
        assert detect.make_views(H, W, hw) == [(h0, w0, 0)]
        assert detect.make_views(H, W, hw, flip=True) == [(h0, w0, 0), (h0, w0, 1)]


def test_make_views_puts_each_mirrored_twin_behind_its_tile():
    plain = detect.make_views(240, 320, 224, tile=True)
    both = detect.make_views(240, 320, 224, tile=True, flip=True)
    assert len(both) == 8 and both[0::2] == plain and both[1::2] == [(h0, w0, 1) for h0, w0, _f in plain]


@pytest.mark.parametrize("H,W,hw", [(240, 320, 224), (9, 11, 4), (120, 136, 112), (4, 4, 4), (5, 4, 4), (13, 29, 4), (449, 225, 224), (7, 23, 7)])
def test_the_tiles_cover_every_pixel(H, W, hw):
    seen = np.zeros((H, W), np.int32)
    views = detect.make_views(H, W, hw, tile=True)
    assert len(views) == -(-H // hw) * -(-W // hw)
    for h0, w0, fl in views:
        assert fl == 0 and 0 <= h0 <= H - hw and 0 <= w0 <= W - hw
        seen[h0:h0 + hw, w0:w0 + hw] += 1
    assert (seen >= 1).all()


def test_too_many_or_bad_views_raise_value_error():
    assert len(detect.make_views(16, 32, 4, tile=True)) == 32                        # exactly the cap
    with pytest.raises(ValueError, match="16 x 36"):
        detect.make_views(16, 36, 4, tile=True)                                       # 4 x 9 tiles
    with pytest.raises(ValueError, match="16 x 32"):
        detect.make_views(16, 32, 4, tile=True, flip=True)
    with pytest.raises(ValueError):
        detect.make_views(100, 320, 224, tile=True)                                   # a frame smaller than the crop
    assert detect.check_views([(2, 3, 0), [5, 7, 1]], 9, 11, 4) == [(2, 3, 0), (5, 7, 1)]
    for bad in ([(6, 0, 0)], [(0, 8, 0)], [(-1, 0, 0)], [(0, -1, 1)], [(0, 0, 2)], [(0, 0, -1)], [], [(0, 0, 0)] * 33, [(0, 0)], 7, [None]):
        with pytest.raises(ValueError):
            detect.check_views(bad, 9, 11, 4)


def _refusals(lib):
    """(entry, argument order, good arguments, [(key, bad value, word of the message)])."""
    vp = C.c_void_p
    st = (C.c_int32 * 32)(*range(32))
    neg = (C.c_int32 * 32)(*([0] * 31 + [-1]))
    good = [(v % 5, v % 4, v & 1) for v in range(32)]

    def table(last):
        return (C.c_int32 * 96)(*[x for r in good[:31] + [last] for x in r])

    shape = [("F", 0, b"outside"), ("S", 0, b"outside"), ("S", 16, b"outside"), ("H", 7, b"outside"), ("W", 7, b"outside")]
    views = [("views", table(last), b"outside") for last in ((5, 2, 0), (2, 5, 0), (-1, 2, 0), (2, -1, 1), (2 ** 31 - 5, 0, 0), (0, 2 ** 31 - 1, 1))] + \
            [("views", table((4, 4, fl)), b"flip") for fl in (2, -1, 256)] + \
            [("V", 0, b"views outside"), ("V", 33, b"views outside"), ("V", -1, b"views outside"), ("view_stride", 1, b"view_stride"),
             ("view_stride", 0, b"view_stride"), ("view_stride", -3, b"view_stride")]
    clips = [("n", 0, b"clips outside"), ("n", 33, b"clips outside"), ("n", -1, b"clips outside"), ("f_skip", 0, b"f_skip"), ("f_skip", -2, b"f_skip"),
             ("starts", neg, b"negative")]
    cut = (lib.pc_clips_from_u8_views, ("video", "F", "H", "W", "S", "views", "V", "view_stride", "starts", "n", "f_skip", "data"),
           dict(video=vp(64), F=20, H=12, W=12, S=8, views=table((4, 4, 1)), V=2, view_stride=2, starts=st, n=2, f_skip=2, data=vp(64)),
           [(k, None, b"null") for k in ("video", "views", "starts", "data")] + shape + views + clips + [("data", vp(68), b"16-byte")])
    merge = (lib.pc_detect_frames_views,
             ("logits", "F", "H", "W", "S", "views", "V", "view_stride", "starts", "n", "f_skip", "row0", "mask", "rec", "ws"),
             dict(logits=vp(64), F=20, H=12, W=12, S=8, views=table((4, 4, 1)), V=2, view_stride=2, starts=st, n=2, f_skip=2, row0=0, mask=vp(64),
                  rec=vp(64), ws=vp(64)),
             [(k, None, b"null") for k in ("logits", "views", "starts", "rec", "ws")] + shape + views + clips +
             [("S", 6, b"multiple of 4"), ("S", 2, b"multiple of 4"), ("logits", vp(68), b"16-byte"), ("logits", vp(72), b"16-byte"),
              ("ws", vp(68), b"aligned"), ("rec", vp(66), b"aligned"), ("row0", -1, b"row0"), ("row0", 2 ** 31 - 1000, b"row0")])
    return cut, merge


def test_bad_arguments_are_refused_without_gpu(built):
    for fn, order, ok, bad in _refusals(built):
        for key, val, word in bad:
            args = dict(ok, **{key: val})
            if key == "starts" and val is not None:
                args["n"] = args["view_stride"] = 32             # the negative start is the last of 32
            if key == "views" and val is not None:
                args["V"] = 32                                   # the bad view is the last of 32
            rc = fn(*[args[k] for k in order], None)
            assert rc == -1, (fn.__name__, key, val, rc)         # PC_E_ARG, before any HIP call (there is no device here to make one on)
            assert word in built.pc_last_error(), (fn.__name__, key, val, built.pc_last_error())
    # the cap of the library (csrc/clipgeom.h) and the one the Python side keeps (ops.MAX_VIEWS, which detect.py takes) are one number
    cap = ops.MAX_VIEWS
    for fn, order, ok, _bad in _refusals(built):
        assert fn(*[dict(ok, V=cap + 1)[k] for k in order], None) == -1 and b"views outside 1..%d" % cap in built.pc_last_error()
    assert ops._view_table([(0, 0, 0)] * cap, "test")[1] == cap and detect.MAX_VIEWS == cap
    with pytest.raises(ValueError, match="1..%d views" % cap):
        ops._view_table([(0, 0, 0)] * (cap + 1), "test")
    frames = built.pc_detect_frames_views
    assert frames(C.c_void_p(64), 20, 1 << 16, 1 << 16, 8, (C.c_int32 * 3)(0, 0, 0), 1, 2, (C.c_int32 * 2)(0, 1), 2, 2, 0, None, C.c_void_p(64),
                  C.c_void_p(64), None) == -1 and b"2^31" in built.pc_last_error()


def test_ws_bytes_of_the_merge(built):
    ws = built.pc_detect_frames_views_ws_bytes
    bad = ((0, 8, 8), (33, 8, 8), (-1, 8, 8), (2, 0, 8), (2, 8, 0), (2, -4, 8), (2, 1 << 16, 1 << 15), (2, 2 ** 31 - 1, 2 ** 31 - 1))
    assert [ws(*a) for a in bad] == [-1] * len(bad)
    # n * 8 frames, min(64, ceil(ceil(H * W / 4) / 1024)) blocks per frame, one 32-byte partial per block
    assert ws(1, 9, 11) == 8 * 32 and ws(3, 120, 136) == 3 * 8 * 4 * 32 and ws(14, 240, 320) == 14 * 8 * 19 * 32
    assert ws(32, 1080, 1920) == 32 * 8 * 64 * 32 and ws(1, 64, 65) == 8 * 2 * 32


def test_header_binding_and_library_agree_on_the_view_entries_at_abi_107(built):
    with open(os.path.join(ROOT, "include", "picons.h")) as f:
        header = f.read()
    assert int(re.search(r"#define\s+PC_VERSION\s+(\d+)", header).group(1)) == 107
    assert capi.ABI_VERSION == 107 and built.pc_version() == 107
    for name in ("pc_clips_from_u8_views", "pc_detect_frames_views", "pc_detect_frames_views_ws_bytes"):
        assert name in capi.EXPORTS and re.search(r"\b%s\(" % name, header), name
        getattr(built, name)


def test_host_side_of_the_view_entries_under_asan_ubsan():
    """Every refusal path of the three entries as a stand-alone program against the sanitizer build of the library (no GPU, nothing loaded
    into Python): tests/detect_views_host_driver.cpp."""
    csrc = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "csrc")
    subprocess.run(["make", "-C", csrc, "-j8", "asan/detect_views_host_driver"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "asan", "detect_views_host_driver")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
