"""GPU: pc_mask_run_index / pc_mask_runs (csrc/maskruns.hip) on their own.  Integer arithmetic: index and runs are exact against the numpy
restatement (tests/mask_runs_ref.py); both buffers sit inside a canary prefill that must stay intact in front of and behind them; a second run
and the outputs the calls allocate themselves are bit-identical.

Block sizes the shapes are chosen around: a block of the count / write kernels takes a band of 32 rows, the one block that scans the band sums
takes 256 bands (8192 rows) per trip, a block of the add-back kernel 256 rows, a wave 256 pixels of a row per segment, a lane 4."""
import numpy as np
import pytest
import torch

from picons_amd import capi, ops

from tests import mask_runs_ref as ref

pytestmark = pytest.mark.gpu
CANARY = -858993460
PAD = 5                                                              # canary words in front of and behind each buffer
SCAN_TRIP_ROWS = 8192


def _device_map(m, odd=False):
    """The map on the device; odd: as a view that starts at an odd byte address."""
    if not odd:
        return torch.from_numpy(m).cuda()
    buf = torch.zeros(m.size + 8, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + m.size].view(m.shape)
    view.copy_(torch.from_numpy(m))
    assert view.data_ptr() % 2 == 1
    return view


def _export(dm, f0, nf, H, cap):
    """index and runs of the range, each between PAD canary words -> (index tensor, runs tensor [cap, 2], the two padded buffers)."""
    ibuf = torch.full((PAD + nf * H + 1 + PAD,), CANARY, dtype=torch.int32, device="cuda")
    index = ibuf[PAD:PAD + nf * H + 1]
    assert ops.mask_run_index(dm, f0, nf, index=index) is index
    rbuf = torch.full((PAD + cap * 2 + PAD,), CANARY, dtype=torch.int32, device="cuda")
    runs = rbuf[PAD:PAD + cap * 2].view(cap, 2)
    assert ops.mask_runs(dm, index, f0, nf, cap=cap, runs=runs) is runs
    return index, runs, ibuf, rbuf


def _check(m, f0=0, nf=None, odd=False, dm=None, want=None, short=()):
    """m uint8 numpy [F,H,W] (dm: the device tensor that holds it, if the test placed it itself; want: (index, runs) if the test states them
    itself).  The range's index and runs are exact over a canary, twice, and so are the tensors the calls allocate; then once more for every
    `short` with cap = total - short."""
    F, H, W = (m.shape if dm is None else tuple(dm.shape))
    nf = F - f0 if nf is None else nf
    want_index, want_runs = ref.runs_of(m[f0:f0 + nf]) if want is None else want
    total = int(want_index[-1])
    assert total == want_runs.shape[0]
    dm = _device_map(m, odd) if dm is None else dm
    index, runs, ibuf, rbuf = _export(dm, f0, nf, H, total)
    got_index, got_runs = index.cpu().numpy(), runs.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_index, want_index), np.flatnonzero(got_index != want_index)[:8].tolist()
    assert np.array_equal(got_runs, want_runs), np.argwhere(got_runs != want_runs)[:8].tolist()
    for buf in (ibuf, rbuf):
        assert (buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all()
    if want is None:
        assert np.array_equal(ops.decode_mask_runs(got_runs, nf, H, W), m[f0:f0 + nf])
    index2, runs2, ibuf2, rbuf2 = _export(dm, f0, nf, H, total)
    assert torch.equal(ibuf2, ibuf) and torch.equal(rbuf2, rbuf)     # the second run: the same bits
    fresh_index = ops.mask_run_index(dm, f0, nf)
    assert fresh_index.shape == index.shape and torch.equal(fresh_index, index)
    fresh_runs = ops.mask_runs(dm, fresh_index, f0, nf)               # cap=None: the total read from the index
    assert fresh_runs.shape == (total, 2) and torch.equal(fresh_runs, runs)
    for less in short:
        cap = total - less
        assert cap >= 0
        i3, r3, ibuf3, rbuf3 = _export(dm, f0, nf, H, cap)
        assert torch.equal(ibuf3, ibuf)                              # the index does not know of the cap: its last word is still the true total
        assert np.array_equal(r3.cpu().numpy().view(np.uint32), want_runs[:cap])
        assert (rbuf3[:PAD] == CANARY).all() and (rbuf3[PAD + cap * 2:] == CANARY).all()
    return want_index, want_runs


def test_one_pixel():
    index, runs = _check(np.zeros((1, 1, 1), np.uint8))               # total 0: cap = 0, an empty runs tensor
    assert index.tolist() == [0, 0] and runs.shape == (0, 2)
    index, runs = _check(np.full((1, 1, 1), 7, np.uint8))
    assert index.tolist() == [0, 1] and runs.tolist() == [[7 << 24, 1 << 16]]


def test_cap_zero_with_a_buffer_writes_nothing():
    m = np.full((1, 2, 9), 3, np.uint8)
    dm = _device_map(m)
    index = ops.mask_run_index(dm)
    assert index.cpu().tolist() == [0, 1, 2]
    buf = torch.full((8,), CANARY, dtype=torch.int32, device="cuda")
    inside = ops.C.c_void_p(buf.data_ptr() + 8)                       # a non-null runs pointer with cap = 0
    capi.call("pc_mask_runs", ops.ptr(dm), 1, 2, 9, 0, 1, ops.ptr(index), 0, inside, ops.stream())
    torch.cuda.synchronize()
    assert (buf == CANARY).all()


def test_five_pixels_by_hand():
    index, runs = _check(np.array([[[3, 3, 0, 3, 4]]], np.uint8))
    assert index.tolist() == [0, 3]
    assert runs.tolist() == [[3 << 24, 0 | 2 << 16], [3 << 24, 3 | 4 << 16], [4 << 24, 4 | 5 << 16]]
    _check(np.array([[[0, 1, 1, 2, 2, 0, 2, 255]]], np.uint8))


def test_odd_address_every_value_class_and_touching_segments():
    m = np.zeros((3, 9, 11), np.uint8)
    m[0, 0] = [1, 1, 2, 2, 2, 255, 255, 0, 254, 1, 1]                # touching segments of different values, up to the row's end
    m[0, 8] = [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9]                      # the last pixel of a frame ...
    m[1, 0] = [9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]                      # ... and the first of the next, the same value: two runs
    m[1, 4] = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]                    # every pixel its own run
    m[2, 3] = 255
    m[2, 4, 3:8] = 128
    m[2, 8, 10] = 1
    assert 3 * 9 * 11 % 2 == 1                                       # frames at odd and even offsets from the odd base
    index, runs = _check(m, odd=True)
    assert index[-1] == 5 + 1 + 1 + 11 + 1 + 1 + 1


def test_lane_and_segment_boundaries_in_a_row_of_1000():
    m = np.zeros((1, 1, 1000), np.uint8)
    row = m[0, 0]
    planted = [(0, 4, 1), (4, 8, 2), (60, 64, 3), (64, 68, 3), (124, 128, 5), (192, 256, 6), (256, 260, 6), (300, 301, 7), (250, 262, 0),
               (508, 512, 8), (512, 516, 9), (640, 768, 10), (768, 772, 11), (996, 1000, 12)]
    for x0, x1, v in planted:
        if v:
            row[x0:x1] = v
    row[250:262] = 13                                                # one run across the segment boundary at 256, over what lay there
    index, runs = _check(m)
    got = [(w1 & 0xffff, w1 >> 16, w0 >> 24) for w0, w1 in runs.tolist()]
    assert (250, 262, 13) in got and (60, 68, 3) in got and (192, 250, 6) in got and (996, 1000, 12) in got and (508, 512, 8) in got


@pytest.mark.parametrize("W", [255, 256, 257, 65535])
def test_a_row_that_is_one_run_of_full_width(W):
    m = np.full((1, 2, W), 200, np.uint8)
    m[0, 1, 0] = 0                                                   # the second row: the run starts at 1
    index, runs = _check(m)
    assert runs.tolist() == [[0 | 200 << 24, 0 | W << 16], [1 | 200 << 24, 1 | W << 16]]


def test_more_runs_than_any_cap_of_the_labelling():
    y, x = np.mgrid[0:64, 0:64]
    checker = ((x + y) % 2).astype(np.uint8)[None]
    index, runs = _check(checker)
    assert index[-1] == 2048
    differs = (1 + (x + y) % 3).astype(np.uint8)[None]                # every pixel differs from its left neighbour and none is zero
    index, runs = _check(differs, short=(1, 7))
    assert index[-1] == 4096


@pytest.mark.parametrize("density", [0.08, 0.5, 0.97])
def test_random_maps(density):
    rng = np.random.default_rng(int(density * 100))
    vals = np.array([1, 2, 3, 255], np.uint8)
    m = vals[rng.integers(0, 4, (4, 37, 53))]
    m[rng.random(m.shape) >= density] = 0
    _check(m, short=(1, 7))
    _check(m, odd=True)


@pytest.mark.parametrize("H", [2049, SCAN_TRIP_ROWS + 1, 2 * SCAN_TRIP_ROWS + 1])
def test_more_rows_than_one_scan_block_takes(H):
    rng = np.random.default_rng(H)
    m = np.array([0, 0, 1, 2], np.uint8)[rng.integers(0, 4, (1, H, 3))]
    m[0, -1] = [1, 0, 1]                                             # the last row, alone in its band, holds two runs
    index, runs = _check(m, short=(1,))
    assert index[-1] - index[-2] == 2


def test_a_range_of_frames_numbers_its_rows_from_the_range():
    rng = np.random.default_rng(5)
    m = np.array([0, 1, 7, 255], np.uint8)[rng.integers(0, 4, (5, 7, 13))]
    want_index, want_runs = _check(m, f0=1, nf=2)
    assert (want_runs[:, 0] & 0xffffff).max() < 2 * 7                # rows of the range, not of the video
    # the other frames are not read: canaries there give the same runs
    dm = torch.full((5, 7, 13), 0xcc, dtype=torch.uint8, device="cuda")
    dm[1:3] = torch.from_numpy(m[1:3]).cuda()
    _check(m, f0=1, nf=2, dm=dm, want=(want_index, want_runs))
    _check(m, f0=4, nf=1, odd=True)                                  # the last frame


def test_the_last_frames_of_a_map_beyond_two_gib():
    """2100 frames of 1024 x 1024: the range (f0 = 2098, nf = 2) starts beyond byte 2^31.  The expectation is written from the planted list."""
    F, H, W = 2100, 1024, 1024
    dm = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
    dm[2097].fill_(0xcc)                                             # the frame in front of the range: not read
    dm[2098:].zero_()
    # (frame of the range, y, x0, x1, value), in raster order
    planted = [(0, 0, 0, 4, 1), (0, 0, 4, 5, 2), (0, 1, 250, 262, 3), (0, 511, 0, 1024, 4), (0, 1023, 1020, 1024, 5),
               (1, 0, 0, 1, 5), (1, 31, 767, 769, 255), (1, 32, 100, 612, 6), (1, 32, 612, 613, 7), (1, 33, 1, 2, 1),
               (1, 1000, 511, 513, 8), (1, 1023, 1023, 1024, 9)]
    for f, y, x0, x1, v in planted:
        dm[2098 + f, y, x0:x1] = v
    assert (2098 * H * W) > 2 ** 31
    want_runs = np.array([((f * H + y) | v << 24, x0 | x1 << 16) for f, y, x0, x1, v in planted], np.uint32)
    per_row = np.zeros(2 * H, np.int64)
    for f, y, _x0, _x1, _v in planted:
        per_row[f * H + y] += 1
    want_index = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)
    _check(None, f0=2098, nf=2, dm=dm, want=(want_index, want_runs), short=(1,))


def test_ops_refuse_what_the_entries_would():
    dm = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    index = ops.mask_run_index(dm)
    for bad in (dict(f0=-1), dict(f0=2), dict(nf=0), dict(nf=3), dict(f0=1, nf=2)):
        with pytest.raises(ValueError):
            ops.mask_run_index(dm, **bad)
        with pytest.raises(ValueError):
            ops.mask_runs(dm, index, **bad)
    with pytest.raises(ValueError):
        ops.mask_run_index(dm.to(torch.int32))
    with pytest.raises(ValueError):
        ops.mask_run_index(dm[:, :, ::2])
    with pytest.raises(ValueError):
        ops.mask_run_index(dm, index=torch.zeros(6, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.mask_runs(dm, index[:-1])
    with pytest.raises(ValueError):
        ops.mask_runs(dm, index, cap=-1)
    with pytest.raises(ValueError):
        ops.mask_runs(dm, index, cap=2, runs=torch.zeros((3, 2), dtype=torch.int32, device="cuda"))
