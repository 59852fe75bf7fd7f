"""GPU: ops.paint_boxes (pc_paint_boxes, csrc/truthboxes.hip) against the numpy restatement tests/truth_boxes_ref.py, byte for byte.  The map is
a view at a byte offset inside a larger allocation filled with 0xAB: the guard bytes in front, behind and in the frames not addressed must
still read 0xAB, and an addressed frame equals the reference (so it shows 0xAB only where a rect of that value painted it).  Frame sizes from
1 x 1 over odd H * W (frames at every byte phase), W < 4 and H * W no multiple of 4 to 240 x 320 (several blocks per frame) and 1080 x 1920
(the cap of 64); R = 1 and R = 32; tables that are empty, whole-frame, single corner pixels, overlapping with a value-0 rect on top, value
255, rects at every byte phase of a four-pixel group, random; binary on and off; frame ranges; determinism.  Every table is valid."""
import numpy as np
import pytest
import torch

from picons_amd import ops
from picons_amd.evalstep import BoxTruth

from tests import truth_boxes_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 0xAB
SIZES = [(1, 1), (3, 5), (5, 7), (7, 3), (9, 1), (6, 7), (120, 136), (240, 320)]
RANGES = [(0, 5), (2, 1), (4, 1), (1, 3)]
OFFSETS = (1, 3, 64)                         # two odd byte offsets and an aligned one (where H * W % 4 == 0 the dword store is taken only there)


def _tables(F, H, W, R):
    """name -> a valid int32 [F, R, 5] table."""
    rng = np.random.default_rng(1000 * H + 10 * W + R + F)
    out = {"empty": np.zeros((F, R, 5), np.int32)}
    whole = np.zeros((F, R, 5), np.int32)
    whole[:, R - 1] = (0, W, 0, H, 5)
    out["whole"] = whole
    px = np.zeros((F, R, 5), np.int32)
    px[0, 0] = (0, 1, 0, 1, 9)
    px[F - 1, R - 1] = (W - 1, W, H - 1, H, 255)                     # (for F = R = 1 this is the one rect: the far corner)
    out["pixels"] = px
    ov = np.zeros((F, R, 5), np.int32)                               # overlapping rects, the last wins; a value-0 rect on top paints nothing
    for f in range(F):
        for r in range(R):
            x0, y0 = (r * 3 + f) % max(W - 1, 1), (r * 2 + f) % max(H - 1, 1)
            ov[f, r] = (x0, min(W, x0 + 1 + W // 2), y0, min(H, y0 + 1 + H // 2), (0, 255, 1 + r, 171)[r % 4] if R > 1 else 255)
    out["overlap"] = ov
    ph = np.zeros((F, R, 5), np.int32)                               # starts and ends at every byte phase of a group of four
    for f in range(F):
        for r in range(R):
            k = f * R + r
            x0 = min(k % 4 + 4 * ((k // 16) % 3), W)
            x1 = min(x0 + 1 + (k // 4) % 4, W)
            y0 = min(k % H, H)
            ph[f, r] = (x0, x1, y0, min(y0 + 1 + k % 3, H), 1 + k % 250)
    out["phases"] = ph
    rd = np.zeros((F, R, 5), np.int64)
    rd[..., 0:2] = np.sort(rng.integers(0, W + 1, (F, R, 2)), axis=2)
    rd[..., 2:4] = np.sort(rng.integers(0, H + 1, (F, R, 2)), axis=2)
    rd[..., 4] = rng.integers(0, 256, (F, R)) * (rng.random((F, R)) < 0.8)
    out["random"] = rd.astype(np.int32)
    for name, t in out.items():
        BoxTruth((F, H, W), t)                                       # every table in this file is valid
    return out


def _paint(rects, F, H, W, f0, nf, binary, offset):
    """-> (the allocation, the view the launch wrote, its bytes in front and behind)."""
    n = F * H * W
    big = torch.full((offset + n + 67,), GUARD, dtype=torch.uint8, device="cuda")
    view = big[offset:offset + n].view(F, H, W)
    got = ops.paint_boxes(torch.from_numpy(rects).cuda(), F, H, W, f0, nf, binary=binary, truth=view)
    assert got.data_ptr() == view.data_ptr()
    return big, view, big[:offset], big[offset + n:]


def _check(rects, F, H, W, f0, nf, binary, offset, want=None):
    want = ref.paint(rects, F, H, W, binary) if want is None else want
    big, view, front, back = _paint(rects, F, H, W, f0, nf, binary, offset)
    assert bool((front == GUARD).all()) and bool((back == GUARD).all())
    got = view.cpu().numpy()
    assert np.array_equal(got[f0:f0 + nf], want[f0:f0 + nf])
    assert (got[:f0] == GUARD).all() and (got[f0 + nf:] == GUARD).all()                       # frames not addressed: untouched
    return want, got


@pytest.mark.parametrize("R", [1, 32])
@pytest.mark.parametrize("H,W", SIZES)
def test_one_frame_every_table(H, W, R):
    for name, rects in _tables(1, H, W, R).items():
        for binary in (False, True):
            want = ref.paint(rects, 1, H, W, binary)
            if name == "whole":
                assert (want == (1 if binary else 5)).all()
            for offset in OFFSETS:
                _check(rects, 1, H, W, 0, 1, binary, offset, want)


@pytest.mark.parametrize("R", [1, 32])
@pytest.mark.parametrize("H,W", SIZES)
def test_five_frames_every_range(H, W, R):
    for name, rects in _tables(5, H, W, R).items():
        if name == "pixels":
            d = ref.paint(rects, 5, H, W)
            assert d[4, H - 1, W - 1] == 255 and d[0, 0, 0] == 9
        for binary in (False, True):
            want = ref.paint(rects, 5, H, W, binary)
            for k, (f0, nf) in enumerate(RANGES):
                _check(rects, 5, H, W, f0, nf, binary, OFFSETS[k % 3], want)


def test_full_hd_blocks_per_frame_at_the_cap():
    F, H, W = 2, 1080, 1920
    for R in (1, 32):
        tabs = _tables(F, H, W, R)
        for name in ("overlap", "phases", "random", "pixels"):
            want = ref.paint(tabs[name], F, H, W)
            _check(tabs[name], F, H, W, 0, 2, False, 1, want)
        _check(tabs["random"], F, H, W, 1, 1, True, 64)
        _check(tabs["empty"], F, H, W, 0, 2, False, 3)


def test_the_last_rect_wins_and_a_zero_value_paints_nothing():
    H, W = 12, 18
    rects = np.zeros((1, 4, 5), np.int32)
    rects[0, 0] = (2, 12, 2, 10, 3)
    rects[0, 1] = (6, 16, 4, 12, 7)
    rects[0, 2] = (0, 18, 0, 12, 0)                                  # value 0 over everything: paints nothing
    rects[0, 3] = (8, 9, 5, 6, 255)
    want, got = _check(rects, 1, H, W, 0, 1, False, 1)
    assert got[0, 3, 3] == 3 and got[0, 5, 7] == 7 and got[0, 5, 8] == 255 and got[0, 11, 15] == 7 and got[0, 0, 0] == 0 and got[0, 2, 2] == 3
    assert set(np.unique(got)) == {0, 3, 7, 255}
    want, got = _check(rects, 1, H, W, 0, 1, True, 3)
    assert set(np.unique(got)) == {0, 1} and got.sum() == (want != 0).sum()


def test_a_second_launch_gives_the_same_bytes():
    for H, W in ((5, 7), (240, 320)):
        rects = _tables(5, H, W, 32)["random"]
        big, view, _f, _b = _paint(rects, 5, H, W, 0, 5, False, 1)
        first = big.clone()
        ops.paint_boxes(torch.from_numpy(rects).cuda(), 5, H, W, 0, 5, truth=view)
        assert torch.equal(big, first)
        ops.paint_boxes(torch.from_numpy(rects).cuda(), 5, H, W, 1, 3, truth=view)               # a range over painted frames: the same bytes again
        assert torch.equal(big, first)


def test_a_fresh_map_is_whole_or_zero_filled_and_operands_are_checked():
    H, W = 6, 7
    rects = _tables(5, H, W, 2)["random"]
    want = ref.paint(rects, 5, H, W)
    d = torch.from_numpy(rects).cuda()
    got = ops.paint_boxes(d, 5, H, W)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, H, W) and np.array_equal(got.cpu().numpy(), want)
    part = ops.paint_boxes(d, 5, H, W, f0=1, nf=2).cpu().numpy()
    assert np.array_equal(part[1:3], want[1:3]) and not part[:1].any() and not part[3:].any()
    for f0, nf in ((-1, 1), (0, 6), (5, 1), (2, 0)):
        with pytest.raises(ValueError, match="paint_boxes"):
            ops.paint_boxes(d, 5, H, W, f0=f0, nf=nf)
    with pytest.raises(ValueError, match="paint_boxes"):
        ops.paint_boxes(d, 4, H, W)                                  # a table of another video
    with pytest.raises(ValueError, match="paint_boxes"):
        ops.paint_boxes(torch.zeros(5, 33, 5, dtype=torch.int32, device="cuda"), 5, H, W)
    with pytest.raises(ValueError, match="paint_boxes"):
        ops.paint_boxes(d, 5, H, W, truth=torch.zeros(5 * H * W - 1, dtype=torch.uint8, device="cuda"))
