"""GPU: pc_frame_instances (ops.frame_instances) against the numpy restatement of tests/instances_ref.py: records exact, imap equal.  Every
launch writes into buffers full of canaries, is repeated without an imap for bit-identical records, and for every input that is not the
overflow case the restatement's own run count is asserted to lie within PC_INST_MAX_RUNS, so that no case passes by falling back."""
import numpy as np
import pytest
import torch

from picons_amd import ops

from tests import instances_ref as ref

pytestmark = pytest.mark.gpu
REC_CANARY, MAP_CANARY = -858993460, 0x5A


def _check(mask, conn=8, min_area=1, K=8, overflow=(), dev_mask=None):
    """mask uint8 numpy [F,H,W] (dev_mask: the device tensor holding it, if the test made one itself) -> the restatement's records."""
    F, H, W = mask.shape
    want, want_map, runs = ref.video_instances(mask, conn, min_area, K)
    for f in range(F):
        assert (runs[f] > ops.INST_MAX_RUNS) == (f in overflow), (f, runs[f])
    dm = torch.from_numpy(mask).cuda() if dev_mask is None else dev_mask
    inst = torch.full((F, ops.INST_HDR + K * ops.INST_WORDS), REC_CANARY, dtype=torch.int32, device="cuda")
    imap = torch.full((F, H, W), MAP_CANARY, dtype=torch.uint8, device="cuda")
    got, got_map = ops.frame_instances(dm, conn=conn, min_area=min_area, K=K, inst=inst, imap=imap)
    assert got is inst and got_map is imap
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert torch.equal(got_map.cpu(), torch.from_numpy(want_map))
    again = torch.full_like(inst, REC_CANARY)                      # a null imap and a second run: bit-identical records
    _r, none = ops.frame_instances(dm, conn=conn, min_area=min_area, K=K, inst=again, want_imap=False)
    assert none is None and torch.equal(again, inst)
    n, kept, n_runs, flags, areas, boxes, first = ops.decode_instances(got, K)
    assert np.array_equal(n_runs, runs) and np.array_equal(kept, np.minimum(n, K)) and np.array_equal(flags, [int(f in overflow) for f in range(F)])
    return want, want_map


def test_one_pixel_on_and_off_and_a_full_square():
    want, _m = _check(np.ones((1, 1, 1), np.uint8))
    assert want[0, :10].tolist() == [1, 1, 1, 0, 1, 0, 0, 1, 1, 0]
    want, _m = _check(np.zeros((1, 1, 1), np.uint8))
    assert not want.any()
    want, m = _check(np.ones((1, 4, 4), np.uint8), K=2)
    assert want[0].tolist() == [1, 1, 4, 0, 16, 0, 0, 4, 4, 0] + [0] * 6 and (m == 1).all()


def test_odd_byte_address_and_blobs_that_touch_only_diagonally():
    F, H, W = 3, 9, 11
    rng = np.random.default_rng(5)
    mask = (rng.random((F, H, W)) < 0.3).astype(np.uint8)
    mask[0] = 0
    mask[0, 1:4, 1:4] = 1
    mask[0, 4:7, 4:7] = 1
    buf = torch.zeros(F * H * W + 7, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + F * H * W].view(F, H, W)
    view.copy_(torch.from_numpy(mask))
    assert view.data_ptr() % 2 == 1 and view.is_contiguous() and (H * W) % 2 == 1          # every frame of it at another alignment
    w4, _m = _check(mask, conn=4, dev_mask=view)
    w8, _m = _check(mask, conn=8, dev_mask=view)
    assert w4[0, :2].tolist() == [2, 2] and w4[0, 4:16].tolist() == [9, 1, 1, 4, 4, 12, 9, 4, 4, 7, 7, 48]
    assert w8[0, :2].tolist() == [1, 1] and w8[0, 4:10].tolist() == [18, 1, 1, 7, 7, 12]


def _spiral(n):
    m = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    free = lambda v, u: not (0 <= v < n and 0 <= u < n) or not m[v, u]
    ahead = lambda: 0 <= y + dy < n and 0 <= x + dx < n and not m[y + dy, x + dx] and free(y + 2 * dy, x + 2 * dx)
    for _ in range(n * n):
        if not ahead():
            dy, dx = dx, -dy
            if not ahead():
                break
        y, x = y + dy, x + dx
        m[y, x] = 1
    return m


def test_labels_travel_against_raster_order_and_along_the_longest_chain():
    mask = np.zeros((2, 16, 16), np.uint8)
    mask[0, 1:15, 2] = mask[0, 1:15, 12] = 1                       # a "U": the arms join only at the bottom row
    mask[0, 14, 2:13] = 1
    mask[0, 3:6, 6:9] = 1                                          # and a blob between the arms that belongs to neither
    mask[1] = _spiral(16)
    assert mask[1].sum() > 100
    for conn in (4, 8):
        want, m = _check(mask, conn=conn)
        assert want[0, :2].tolist() == [2, 2] and want[0, 4:10].tolist() == [14 + 14 + 9, 2, 1, 13, 15, 16 + 2]
        assert want[1, :2].tolist() == [1, 1] and want[1, 4] == mask[1].sum() and want[1, 2] > 16      # one component through every run
        assert (m[1][mask[1] != 0] == 1).all()


def test_runs_across_every_thread_and_wave_chunk_of_a_long_row():
    mask = np.zeros((1, 3, 1000), np.uint8)
    mask[0, 0] = 7                                                 # a full row is one run
    runs = [(0, 4), (5, 8), (60, 64), (65, 128), (129, 256), (257, 260), (508, 516), (636, 640), (700, 768), (769, 1000)]
    for a, b in runs:
        mask[0, 2, a:b] = 1
    want, _m = _check(mask, K=32)
    assert want[0, :3].tolist() == [1 + len(runs), 1 + len(runs), 1 + len(runs)] and want[0, 4:10].tolist() == [1000, 0, 0, 1000, 1, 0]
    got = sorted((int(r[1]), int(r[3])) for r in want[0, 4:].reshape(32, 6)[1:1 + len(runs)])
    assert got == runs
    mask[0, 1, [3, 4, 63, 64, 255, 256, 511, 512, 999]] = 1        # single pixels at the chunk boundaries join what they touch
    # 4-connected they reach the runs below them; 8-connected also those that start one column on: (636, 640) and (700, 768) stay alone
    for conn, n_comp, joined in ((4, 6, [(0, 4), (60, 64), (129, 256), (508, 516), (769, 1000)]), (8, 3, [r for r in runs if r[0] not in (636, 700)])):
        want, _m = _check(mask, conn=conn, K=32)
        assert want[0, 0] == n_comp and want[0, 4] == 1000 + 9 + sum(b - a for a, b in joined)


def test_checkerboard_at_the_cap_and_over_it():
    y, x = np.mgrid[0:64, 0:66]
    board = ((y + x) % 2 == 0).astype(np.uint8)
    at_cap = np.ascontiguousarray(board[None, :, :64])
    want, m = _check(at_cap, conn=4, K=8)                          # 2048 runs: at the cap, not over it
    assert want[0, :4].tolist() == [2048, 8, 2048, 0]
    assert want[0, 4:].reshape(8, 6).tolist() == [[1, 2 * i, 0, 2 * i + 1, 1, 2 * i] for i in range(8)]
    assert (m[0][at_cap[0] != 0] == 255).sum() == 2040
    want, m = _check(at_cap, conn=8, K=8)
    assert want[0, :10].tolist() == [1, 1, 2048, 0, 2048, 0, 0, 64, 64, 0] and np.array_equal(m[0], at_cap[0])
    # 2112 runs, the one overflow case, between two frames of the same launch that are not
    rng = np.random.default_rng(11)
    three = np.stack([(rng.random((64, 66)) < 0.1).astype(np.uint8), board, (rng.random((64, 66)) < 0.2).astype(np.uint8)])
    for conn in (4, 8):
        want, m = _check(three, conn=conn, K=8, overflow=(1,))
        assert want[1].tolist() == [0, 0, 2112, 1] + [0] * 48 and np.array_equal(m[1], board * 255)
        assert want[0, 0] > 8 and want[2, 0] > 8 and want[0, 3] == want[2, 3] == 0


@pytest.fixture(scope="module")
def random_masks():
    rng = np.random.default_rng(29)
    return {d: (rng.random((4, 37, 53)) < d).astype(np.uint8) for d in (0.05, 0.3, 0.5)}


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("min_area", (1, 5))
@pytest.mark.parametrize("K", (1, 8, 32))
@pytest.mark.parametrize("density", (0.05, 0.3, 0.5))
def test_random_masks(random_masks, density, K, min_area, conn):
    mask = random_masks[density]
    want, m = _check(mask, conn=conn, min_area=min_area, K=K)
    n, kept, _runs, _flags, areas, _boxes, first = ops.decode_instances(want, K)
    fg = mask != 0
    assert ((m != 0) == fg).all() and all(int(((m[f] > 0) & (m[f] < 255)).sum()) == int(areas[f].sum()) for f in range(4))
    if K == 1 and min_area == 1:
        assert (n > 1).all() and (m == 255).any()                  # components beyond K
    if (density, min_area, conn) == (0.05, 5, 4):
        assert (n == 0).all() and (m[fg] == 255).all()             # everything filtered
    if min_area == 1 and K == 32 and density <= 0.3:
        a = areas[0][:kept[0]]
        ties = np.flatnonzero(a[1:] == a[:-1])
        assert ties.size and (first[0][ties] < first[0][ties + 1]).all()           # equal areas: the earlier first pixel ranks first


def test_empty_frames_and_any_non_zero_byte_is_foreground():
    want, m = _check(np.zeros((2, 5, 7), np.uint8))
    assert not want.any() and not m.any()
    mask = np.zeros((1, 6, 9), np.uint8)
    mask[0, 1, 1:4] = (2, 255, 128)
    mask[0, 4, 5] = 2
    mask[0, 3, 8] = 255
    want, _m = _check(mask, K=4)
    assert want[0, :2].tolist() == [3, 3] and want[0, 4:10].tolist() == [3, 1, 1, 4, 2, 10]


def test_a_sub_range_writes_its_frames_and_nothing_else():
    F, H, W, K, pad = 4, 13, 17, 4, 64
    words = ops.INST_HDR + K * ops.INST_WORDS
    rng = np.random.default_rng(3)
    mask = (rng.random((F, H, W)) < 0.3).astype(np.uint8)
    want, want_map, runs = ref.video_instances(mask, 8, 2, K)
    assert runs.max() <= ops.INST_MAX_RUNS
    ibuf = torch.full((pad + F * words + pad,), REC_CANARY, dtype=torch.int32, device="cuda")
    mbuf = torch.full((pad + F * H * W + pad,), MAP_CANARY, dtype=torch.uint8, device="cuda")
    inst, imap = ibuf[pad:pad + F * words].view(F, words), mbuf[pad:pad + F * H * W].view(F, H, W)
    ops.frame_instances(torch.from_numpy(mask).cuda(), f0=1, nf=2, conn=8, min_area=2, K=K, inst=inst, imap=imap)
    got, got_map = inst.cpu().numpy(), imap.cpu().numpy()
    assert np.array_equal(got[1:3], want[1:3]) and np.array_equal(got_map[1:3], want_map[1:3])
    assert (got[[0, 3]] == REC_CANARY).all() and (got_map[[0, 3]] == MAP_CANARY).all()
    ib, mb = ibuf.cpu().numpy(), mbuf.cpu().numpy()
    assert (ib[:pad] == REC_CANARY).all() and (ib[-pad:] == REC_CANARY).all() and (mb[:pad] == MAP_CANARY).all() and (mb[-pad:] == MAP_CANARY).all()
    with pytest.raises(RuntimeError, match="f0"):
        ops.frame_instances(torch.from_numpy(mask).cuda(), f0=3, nf=2, inst=inst, imap=imap, K=K)
    with pytest.raises(ValueError):
        ops.frame_instances(torch.from_numpy(mask).cuda(), K=33)


def test_one_frame_beyond_byte_2_to_the_31():
    """The last frame of 2100 frames of 1024 x 1024: more than 2^31 bytes into mask and imap.  Only that frame is filled and looked at."""
    F, H, W, K, f = 2100, 1024, 1024, 8, 2099
    assert f * H * W > 2 ** 31
    frame = np.zeros((H, W), np.uint8)
    frame[10:200, 20:300] = 1
    frame[150:400, 290:310] = 1                                    # joins the first
    frame[600:1024, 1000:1024] = 1
    frame[500, 0:1024:2] = 1                                       # 512 single pixels
    frame[900:1000:3, 100:900] = 1                                 # long runs, apart
    frame[1023, 0] = 1
    mask = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    imap = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    mask[f].copy_(torch.from_numpy(frame))
    imap[f - 1].fill_(MAP_CANARY)
    inst = torch.full((F, ops.INST_HDR + K * ops.INST_WORDS), REC_CANARY, dtype=torch.int32, device="cuda")
    want, want_map, n_runs = ref.frame_instances(frame, 8, 2, K)
    assert n_runs <= ops.INST_MAX_RUNS
    ops.frame_instances(mask, f0=f, nf=1, conn=8, min_area=2, K=K, inst=inst, imap=imap)
    got = inst.cpu().numpy()
    assert np.array_equal(got[f], want), (got[f].tolist(), want.tolist())
    assert torch.equal(imap[f].cpu(), torch.from_numpy(want_map))
    assert (got[:f] == REC_CANARY).all() and bool((imap[f - 1] == MAP_CANARY).all())
