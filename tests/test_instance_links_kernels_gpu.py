"""GPU: pc_instance_overlaps (csrc/instances.hip) on its own.  Integer arithmetic: every record is exact against the numpy restatement
(tests/instance_links_ref.py), every addressed cell is written over a canary, nothing else is, and a second run gives the same bits.  Two
invariants on top: a row of a record sums to no more than the pixels of its slot in the first frame, and a whole record to the pixels that are
foreground in both frames."""
import numpy as np
import pytest
import torch

from picons_amd import ops

from tests import instance_links_ref as ref

pytestmark = pytest.mark.gpu
CANARY = -858993460


def _check(imap, K, L, dev=None):
    """imap uint8 numpy [F,H,W] (dev: the device tensor that holds it, if the test placed it itself) -> the restatement's overlaps; the kernel's
    record over a canary is exact against it, twice, and so is the fresh tensor the call makes itself."""
    F = imap.shape[0]
    want = ref.overlaps(imap, K, L)
    di = torch.from_numpy(imap).cuda() if dev is None else dev
    out = torch.full((F, L, K + 1, K + 1), CANARY, dtype=torch.int32, device="cuda")
    assert ops.instance_overlaps(di, K, L, out=out) is out
    got = out.cpu().numpy()
    assert (got != CANARY).all()                                     # every cell of every addressed record is written, the zero lags included
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(ops.decode_instance_overlaps(got.reshape(-1), K, L), want)
    again = torch.full_like(out, CANARY)
    ops.instance_overlaps(di, K, L, out=again)
    assert torch.equal(again, out)
    fresh = ops.instance_overlaps(di, K, L)
    assert fresh.shape == out.shape and torch.equal(fresh, out)
    # the invariants, on what the kernel gave
    pix, fg = ref.slot_pixels(imap, K), (imap != 0).reshape(F, -1)
    for f in range(F):
        for lag in range(L):
            g = f + lag + 1
            if g >= F:
                assert not got[f, lag].any()
                continue
            assert (got[f, lag].sum(1) <= pix[f]).all() and (got[f, lag].sum(0) <= pix[g]).all()
            assert got[f, lag].sum() == np.count_nonzero(fg[f] & fg[g])
    return want


def _random_map(rng, shape, K, density):
    """Every kind of value -- 0, 1..K, K + 1..254, 255 -- as runs of one value (a thread stays in a pair for a while) and as single pixels (it
    changes pair at every pixel)."""
    pool = np.array(list(range(1, K + 1)) + [255] + ([K + 1, 254, (K + 255) // 2] if K + 1 <= 254 else []), np.uint8)
    single = pool[rng.integers(0, pool.size, shape)]
    blocks = pool[rng.integers(0, pool.size, (shape[0], (shape[1] + 7) // 8, (shape[2] + 15) // 16))]
    coarse = np.repeat(np.repeat(blocks, 8, axis=1), 16, axis=2)[:, :shape[1], :shape[2]]
    imap = np.where(rng.random(shape) < 0.5, coarse, single)
    return np.where(rng.random(shape) < density, imap, 0).astype(np.uint8)


def _with_every_value(rng, imap, K):
    """The map with each of 1..K, K + 1, 254 and 255 planted at a pixel of its own (a small map does not draw all of them by itself)."""
    vals = np.array(list(range(1, K + 1)) + [K + 1, 254, 255], np.uint8)
    flat = imap.copy().reshape(-1)
    flat[rng.permutation(flat.size)[:vals.size]] = vals
    return flat.reshape(imap.shape)


def test_one_frame_of_one_pixel_is_a_zero_record():
    want = _check(np.array([[[1]]], np.uint8), K=1, L=1)
    assert want.shape == (1, 1, 2, 2) and not want.any()


def test_two_frames_of_one_pixel():
    want = _check(np.array([[[1]], [[1]]], np.uint8), K=1, L=1)
    assert want[0, 0].tolist() == [[1, 0], [0, 0]] and not want[1].any()
    want = _check(np.array([[[1]], [[2]]], np.uint8), K=1, L=1)                 # a value beyond K: the other slot
    assert want[0, 0].tolist() == [[0, 1], [0, 0]]
    want = _check(np.array([[[255]], [[0]], [[7]]], np.uint8), K=8, L=2)
    assert not want[0, 0].any() and want[0, 1, 8, 6] == 1 and want[0, 1].sum() == 1


@pytest.fixture(scope="module")
def odd_maps():
    rng = np.random.default_rng(11)
    return {K: _with_every_value(rng, _random_map(rng, (3, 9, 11), K, 0.7), K) for K in (1, 8, 32)}


@pytest.mark.parametrize("L", (1, 2, 3, 4))
@pytest.mark.parametrize("K", (1, 8, 32))
def test_odd_byte_address_and_odd_frame_size(odd_maps, K, L):
    """3 x 9 x 11 from an odd address: H * W = 99 is odd, so the three frames sit at three different places in their dwords and the two frames
    of a pair never share an alignment.  L > F - 1 = 2 gives lags without a later frame: zeros."""
    F, H, W = 3, 9, 11
    imap = odd_maps[K]
    assert (imap == 0).any() and (imap == 255).any() and ((imap > K) & (imap < 255)).any() and all((imap == r + 1).any() for r in range(K))
    buf = torch.zeros(F * H * W + 7, dtype=torch.uint8, device="cuda")
    di = buf[1:1 + F * H * W].view(F, H, W)
    di.copy_(torch.from_numpy(imap))
    assert di.data_ptr() % 2 == 1 and (H * W) % 2 == 1
    want = _check(imap, K, L, dev=di)
    assert want[0, 0].any() and want[1, 0].any() and (L < 2 or want[0, 1].any())
    assert not want[2].any() and (L < 2 or not want[1, 1:].any()) and (L < 3 or not want[0, 2:].any())
    assert want[:, :, K, :].any() and want[:, :, :, K].any() and want[:, :, :K, :K].any()


@pytest.mark.parametrize("density,K,L", ((0.08, 8, 1), (0.5, 32, 2), (0.97, 3, 4)))
def test_random_maps(density, K, L):
    """4 x 37 x 53: 1961 pixels, 491 groups of four and one pixel over -- more than one group per thread only at the stride's start, an odd
    frame size, and at the low density most groups of the first frame are background, so their partners are never fetched."""
    rng = np.random.default_rng(int(density * 100) + K)
    imap = _random_map(rng, (4, 37, 53), K, density)
    want = _check(imap, K, L)
    assert want[0, 0].any() and want[2, 0].any() and not want[3].any()


def test_more_than_one_round_of_groups_per_thread():
    """2 x 70 x 130: 2275 groups, so threads walk three rounds of their four-group stride and the last round is partly beyond the frame."""
    rng = np.random.default_rng(4)
    imap = _random_map(rng, (2, 70, 130), 5, 0.6)
    _check(imap, 5, 1)


def test_a_sub_range_writes_its_frames_and_reads_a_partner_outside_it():
    F, H, W, K, L, pad = 5, 13, 17, 4, 2, 64
    words = L * (K + 1) ** 2
    rng = np.random.default_rng(3)
    imap = _random_map(rng, (F, H, W), K, 0.6)
    want = ref.overlaps(imap, K, L)
    obuf = torch.full((pad + F * words + pad,), CANARY, dtype=torch.int32, device="cuda")
    out = obuf[pad:pad + F * words].view(F, L, K + 1, K + 1)
    di = torch.from_numpy(imap).cuda()
    ops.instance_overlaps(di, K, L, f0=1, nf=2, out=out)
    got, ob = out.cpu().numpy(), obuf.cpu().numpy()
    assert np.array_equal(got[1:3], want[1:3]) and (got[[0, 3, 4]] == CANARY).all()
    assert (ob[:pad] == CANARY).all() and (ob[-pad:] == CANARY).all()
    assert want[2, 0].any() and want[2, 1].any()                    # frame 2 against frames 3 and 4: both outside the range, both read
    # the last frame alone: it has no partner, its record is zeros
    ops.instance_overlaps(di, K, L, f0=4, nf=1, out=out)
    got = out.cpu().numpy()
    assert not got[4].any() and (got[[0, 3]] == CANARY).all()
    with pytest.raises(RuntimeError, match="f0"):
        ops.instance_overlaps(di, K, L, f0=4, nf=2, out=out)
    with pytest.raises(ValueError):
        ops.instance_overlaps(di, 33, L)
    with pytest.raises(ValueError):
        ops.instance_overlaps(di, K, 5)
    with pytest.raises(ValueError):
        ops.instance_overlaps(di, K, L, out=out[:4])
    with pytest.raises(ValueError):
        ops.instance_overlaps(di.to(torch.int32), K, L)


def test_a_count_beyond_16_bits():
    H, W = 257, 256
    want = _check(np.ones((2, H, W), np.uint8), K=2, L=1)
    assert want[0, 0, 0, 0] == 65792 > 2 ** 16 and want[0, 0].sum() == 65792


def test_a_pair_of_frames_beyond_byte_2_to_the_31():
    """The last two of 2100 frames of 1024 x 1024: both more than 2^31 bytes into the map.  Only those two are filled and looked at; the
    second lag of the first has no later frame."""
    F, H, W, K, L, f = 2100, 1024, 1024, 8, 2, 2098
    assert f * H * W > 2 ** 31
    pair = np.zeros((2, H, W), np.uint8)
    pair[0, 10:200, 20:300], pair[1, 50:260, 100:400] = 1, 2
    pair[0, 600:1024, 1000:1024], pair[1, 500:1024, 990:1010] = 2, 1
    pair[0, 500, 0:1024:2], pair[1, 500, 0:1024:3] = 3, 255
    pair[0, 900:1000:3, 100:900], pair[1, 880:1000, 500:503] = 255, 9
    pair[0, 1023, 0], pair[1, 1023, 0] = 8, 8
    want = ref.overlaps(pair, K, L)
    assert want[0, 0, 0, 1] == 150 * 200 and want[0, 0, 7, 7] == 1 and want[0, 0, 8, 8] > 0 and not want[0, 1].any() and not want[1].any()
    imap = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    imap[f:f + 2].copy_(torch.from_numpy(pair))
    out = torch.full((F, L, K + 1, K + 1), CANARY, dtype=torch.int32, device="cuda")
    ops.instance_overlaps(imap, K, L, f0=f, nf=2, out=out)
    got = out.cpu().numpy()
    assert np.array_equal(got[f:f + 2], want), np.argwhere(got[f:f + 2] != want)[:8].tolist()
    assert (got[:f] == CANARY).all()
