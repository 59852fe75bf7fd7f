"""GPU: pc_prob_cut (csrc/probcut.hip) through ops.prob_cut, equal to the numpy restatement (tests/prob_cut_ref.py) bit for bit: the mask
q >= word, the count, the half-open box and the float32 score.  Mask, records and workspace are filled with 0xa5 in front of every call --
nothing has to be zeroed, frames outside f0 / nf keep theirs, and so do words 6 and 7 of the addressed records.  The shapes: one pixel, odd
H * W (frames at every 2-byte phase of an 8-byte word: the wide load and the element loads, tail groups), more than one stride of a thread,
a frame of several blocks (the records kernel adds partials) and 1080 x 1920 (the cap of 64 blocks a frame).  The words: the lowest, a half,
the highest and one between.  The maps: coarse blocks above noise with the word and the word - 1 planted side by side and at the corners, a
single positive pixel at each corner, all 0, all 65535, all word - 1."""
import numpy as np
import pytest
import torch

from picons_amd import ops

from tests import prob_cut_ref as ref

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (5, 120, 136), (1, 1080, 1920)]
WORDS = [1, 32768, 65535, 22938]
CANARY = -1515870811                                                                         # 0xa5a5a5a5
_cache = {}


def _to_device(prob, off=1):
    """A host uint16 map on the device, `off` elements into its allocation."""
    buf = torch.zeros(prob.size + 8, dtype=torch.int16, device="cuda")
    buf[off:off + prob.size].copy_(torch.from_numpy(prob.view(np.int16)).reshape(-1))
    return buf[off:off + prob.size].view(prob.shape)


def _maps(shape, word):
    """The map of (shape, word) on the host and on the device (at an odd ELEMENT offset of its allocation), made once.  Upper half of a
    frame: coarse blocks of word - 1, word, 0, 65535 and noise values; lower half: noise, half of it 0, with word and word - 1 planted side
    by side; word, word - 1, word, word - 1 at the four corners."""
    if (shape, word) not in _cache:
        F, H, W = shape
        rng = np.random.default_rng(sum(shape) + word)
        sp = np.array([word - 1, word, 0, 65535, min(word + 1, 65535), word // 2], np.uint16)
        noise = rng.integers(0, 65536, shape).astype(np.uint16)
        noise[rng.random(shape) < 0.5] = 0
        pair = rng.random(shape) < 0.15
        noise[pair] = word
        noise[:, :, 1:][pair[:, :, :-1]] = word - 1                  # (a pair that follows a pair leaves word - 1, word - 1: fine)
        coarse = sp[rng.integers(0, sp.size, (F, -(-H // 7), -(-W // 13)))]
        blocks = np.repeat(np.repeat(coarse, 7, axis=1), 13, axis=2)[:, :H, :W]
        upper = np.arange(H)[None, :, None] < H // 2
        prob = np.ascontiguousarray(np.where(upper, blocks, noise))
        prob[:, 0, 0], prob[:, 0, W - 1], prob[:, H - 1, 0], prob[:, H - 1, W - 1] = word, word - 1, word, word - 1
        if H * W == 1:                                               # the one pixel is all four corners
            prob[:] = word
        _cache[(shape, word)] = (prob, _to_device(prob))
    return _cache[(shape, word)]


def _call(prob, word, f0=0, nf=None, want_mask=True):
    """-> (mask uint8 [F,H,W] host or None, rec int32 [F,8] host); every buffer pre-filled with 0xa5, the mask at an odd byte offset."""
    F, H, W = prob.shape
    mbuf = torch.full((F * H * W + 8,), 0xa5, dtype=torch.uint8, device="cuda")
    mask = mbuf[3:3 + F * H * W].view(F, H, W) if want_mask else None
    rec = torch.full((F, 8), CANARY, dtype=torch.int32, device="cuda")
    ws = torch.full((ops.prob_cut_ws_bytes(F - f0 if nf is None else nf, H, W),), 0xa5, dtype=torch.uint8, device="cuda")
    gm, gr = ops.prob_cut(prob, word, f0=f0, nf=nf, mask=mask, rec=rec, ws=ws, want_mask=want_mask)
    assert gr is rec and (gm is mask if want_mask else gm is None)
    if want_mask:
        assert mask.data_ptr() % 2 == 1
        assert (mbuf[:3] == 0xa5).all() and (mbuf[3 + F * H * W:] == 0xa5).all()
    return (mask.cpu().numpy() if want_mask else None), rec.cpu().numpy()


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_and_records_equal_the_restatement(shape, word):
    hp, dp = _maps(shape, word)
    assert dp.data_ptr() % 4 == 2
    wm, wr = ref.cut(hp, word)
    gm, gr = _call(dp, word)
    assert gm.dtype == np.uint8 and np.array_equal(gm, wm)
    assert np.array_equal(gr[:, :6], wr)
    assert (gr[:, 6:] == CANARY).all()                       # words 6 and 7 are the detect entries'
    assert (wr[:, 0] > 0).all()                              # (the map does hold positive pixels in every frame)
    nm, nr = _call(dp, word, want_mask=False)                # records only: the same bits
    assert nm is None and np.array_equal(nr, gr)
    gm2, gr2 = _call(dp, word)                               # the same bits from a second run
    assert np.array_equal(gm2, gm) and np.array_equal(gr2, gr)


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 120, 136)])
def test_a_sub_range_leaves_the_other_frames_and_words_six_and_seven_alone(shape, word):
    hp, dp = _maps(shape, word)
    F = shape[0]
    wm, wr = ref.cut(hp, word)
    for want_mask in (True, False):
        gm, gr = _call(dp, word, f0=1, nf=F - 2, want_mask=want_mask)
        assert (gr[0] == CANARY).all() and (gr[F - 1] == CANARY).all() and (gr[1:F - 1, 6:] == CANARY).all()
        assert np.array_equal(gr[1:F - 1, :6], wr[1:F - 1])
        if want_mask:
            assert (gm[0] == 0xa5).all() and (gm[F - 1] == 0xa5).all() and np.array_equal(gm[1:F - 1], wm[1:F - 1])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_single_positive_pixel_at_each_corner(shape):
    """Frame f of four holds its one pixel at corner f: the box is that pixel's, half-open, and the score its word / 65535."""
    _F, H, W = shape
    word = 40000
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    hp = np.full((4, H, W), word - 1, np.uint16)
    for f, (y, x) in enumerate(corners):
        hp[f, y, x] = word + f
    gm, gr = _call(_to_device(hp), word)
    wm, wr = ref.cut(hp, word)
    assert np.array_equal(gm, wm) and np.array_equal(gr[:, :6], wr) and (gr[:, 6:] == CANARY).all()
    for f, (y, x) in enumerate(corners):
        assert gr[f, :5].tolist() == [1, x, y, x + 1, y + 1]
        assert gr[f, 5:6].view(np.float32)[0] == np.float32(np.float64(word + f) / 65535.0)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 33, 31), (5, 120, 136), (1, 1080, 1920)])
def test_constant_maps(shape):
    F, H, W = shape
    one = int(np.array([1.0], np.float32).view(np.int32)[0])
    for pv, word, full in ((0, 1, False), (0, 32768, False), (65535, 65535, True), (65535, 1, True), (32767, 32768, False), (32768, 32768, True),
                           (0, 65535, False), (65534, 65535, False), (22937, 22938, False)):
        prob = torch.full(shape, pv - 65536 if pv > 32767 else pv, dtype=torch.int16, device="cuda")
        gm, gr = _call(prob, word)
        want = np.zeros((F, 6), np.int32)
        if full:
            score = np.float32(np.float64(pv * H * W) / (65535.0 * (H * W)))
            want[:] = [H * W, 0, 0, W, H, int(np.array([score], np.float32).view(np.int32)[0])]
        assert np.array_equal(gr[:, :6], want), (pv, word)
        assert (gm == int(full)).all() and (gr[:, 6:] == CANARY).all()
        if pv == 65535:
            assert (gr[:, 5] == one).all()                   # exactly 1.0f
        if not full:
            assert not gr[:, :6].any()                       # count 0, box zeros, the bits of 0.0f


def test_frames_at_every_phase_of_an_eight_byte_word():
    """H * W = 35 is odd and 3 mod 4: the four frames start 0, 6, 4 and 2 bytes into an 8-byte word from an aligned base, and elsewhere from a
    base moved by one, two and three elements."""
    hp, _dp = _maps((3, 5, 7), 22938)
    hp4 = np.concatenate([hp, hp[:1]])
    wm, wr = ref.cut(hp4, 22938)
    for off in range(4):
        dp = _to_device(hp4, off)
        assert dp.data_ptr() % 8 == 2 * off
        gm, gr = _call(dp, 22938)
        assert np.array_equal(gm, wm) and np.array_equal(gr[:, :6], wr), off


def test_fresh_tensors_are_zero_filled_and_arguments_are_checked():
    hp, dp = _maps((3, 5, 7), 32768)
    wm, wr = ref.cut(hp, 32768)
    mask, rec = ops.prob_cut(dp, 32768, f0=1, nf=1)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (3, 5, 7) and rec.dtype == torch.int32 and tuple(rec.shape) == (3, 8)
    m, r = mask.cpu().numpy(), rec.cpu().numpy()
    assert not m[0].any() and not m[2].any() and not r[0].any() and not r[2].any() and not r[1, 6:].any()
    assert np.array_equal(m[1], wm[1]) and np.array_equal(r[1, :6], wr[1])
    none, rec2 = ops.prob_cut(dp, np.int64(32768), want_mask=False)
    assert none is None and np.array_equal(rec2.cpu().numpy()[:, :6], wr)
    counts, boxes, scores, _rows = ops.decode_detect_records(rec2)
    assert np.array_equal(counts, wr[:, 0]) and np.array_equal(boxes, wr[:, 1:5]) and np.array_equal(np.asarray(scores, np.float32).view(np.int32), wr[:, 5])
    if hasattr(torch, "uint16"):
        assert np.array_equal(ops.prob_cut(dp.view(torch.uint16), 32768)[1].cpu().numpy()[:, :6], wr)
    mask = torch.zeros(3, 5, 7, dtype=torch.uint8, device="cuda")
    rec = torch.zeros(3, 8, dtype=torch.int32, device="cuda")
    for kw in (dict(word=0), dict(word=65536), dict(word=-1), dict(word=0.5), dict(word=32768.0), dict(word=True), dict(word=None), dict(word="1"),
               dict(word=[32768]), dict(f0=-1), dict(nf=0), dict(f0=1, nf=3), dict(f0=3),
               dict(mask=mask[:2]), dict(mask=mask.to(torch.int8)), dict(mask=mask.cpu()), dict(mask=mask[:, :, :6]), dict(mask=mask.cpu().numpy()),
               dict(rec=rec[:2]), dict(rec=rec.float()), dict(rec=rec.cpu()), dict(rec=rec[:, :6]), dict(rec=torch.zeros(3, 6, dtype=torch.int32, device="cuda")),
               dict(ws=torch.zeros(8, dtype=torch.uint8, device="cuda")), dict(ws=torch.zeros(4096, dtype=torch.int32, device="cuda")),
               dict(ws=torch.zeros(4096, dtype=torch.uint8))):
        args = dict(word=32768)
        args.update(kw)
        with pytest.raises(ValueError, match="prob_cut"):
            ops.prob_cut(dp, **args)
    for bad in (dp.cpu().numpy(), dp.to(torch.int32), dp.to(torch.uint8), dp[:, :, :5], dp[0], dp.cpu()):
        with pytest.raises(ValueError, match="prob_cut"):
            ops.prob_cut(bad, 32768)
    assert not mask.any() and not rec.any()                  # nothing was launched
