"""GPU: the two kernels of the per-instance confidence on their own (pc_frame_probs in csrc/detect.hip, pc_instance_scores in
csrc/instances.hip).

pc_frame_probs at the shapes, views, launches and logits of tests/test_detect_views_kernels_gpu.py, with 0.0, -0.0, +-80 and +-inf planted as
MERGED logits on top (every view that covers the pixel holds the value): those give exactly 32768 / 65535 / 0, a NaN and an uncovered pixel
0, and every other pixel lies within tests/instance_scores_ref.q_bound of float64 -- a bound put together from the rounding to an integer,
the fp32 product's spacing and the rule the frame scores are held to, not from what the kernel gives; the largest distance seen is printed.
Canaries in front of and behind the map and in the frames a launch does not address; a second run is bit-identical.

pc_instance_scores is integer arithmetic: exact against the restatement."""
import numpy as np
import pytest
import torch

from picons_amd import ops

from tests import instance_scores_ref as ref
from tests.detectviews_ref import real_frames
from tests.test_detect_views_kernels_gpu import MERGE_CASES, _covering, _logits

pytestmark = pytest.mark.gpu
PROB_CANARY, OUT_CANARY = 0x5A5A, -858993460
PLANTS = ((0.0, 32768), (-0.0, 32768), (80.0, 65535), (-80.0, 0), (np.inf, 65535), (-np.inf, 0))


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda()


# ---------------------------------------------------------------------- pc_frame_probs
@pytest.mark.parametrize("F,H,W,S,views,pad,launches", MERGE_CASES)
def test_frame_probs_against_float64(F, H, W, S, views, pad, launches):
    V = len(views)
    assert (F, H, W, S, V) in ((1, 4, 4, 4, 1), (3, 9, 11, 4, 18), (17, 10, 12, 8, 8), (40, 12, 12, 8, 2))
    xs, planted, _box = _logits(launches, views, F, H, W, S, seed=F * 100 + W)
    # the planted merged logits: the covered pixels from the end of the first real frame, behind the two the views test has taken there
    cover = np.zeros((H, W), bool)
    for h0, w0, _fl in views:
        cover[h0:h0 + S, w0:w0 + S] = True
    spots = list(zip(*np.nonzero(cover)))[::-1][2 if V > 1 else 0:][:len(PLANTS)]
    i0, c0, k0, f0 = [(i, c, k, f) for i, st in enumerate(launches) for c, k, f in real_frames(st, F)][0]
    for (y, x), (val, _q) in zip(spots, PLANTS):
        for v, r, q in _covering(views, S, y, x):
            xs[i0][v, c0, k0, r, q] = val
    m = ref.Merge(F, H, W, S)
    for x, st in zip(xs, launches):
        m.add(x, views, st)
    merged, num = m.merged(), m.num
    for (y, x), (val, _q) in zip(spots, PLANTS):
        assert merged[f0, y, x] == val and np.signbit(merged[f0, y, x]) == np.signbit(val)
    assert np.isnan(merged[f0]).any()

    buf = torch.full((pad + F * H * W + 16,), PROB_CANARY, dtype=torch.int16, device="cuda")
    prob = buf[pad:pad + F * H * W].view(F, H, W)
    assert prob.data_ptr() % 8 == (2 * pad) % 8 and (pad != 13 or (prob.data_ptr() // 2) % 2 == 1)       # 13: the map starts at an odd element
    xd = [torch.from_numpy(x).cuda() for x in xs]
    done = set()
    for x, st in zip(xd, launches):
        assert ops.frame_probs(x, views, st, F, H, W, prob=prob) is prob
        done |= {f for _c, _k, f in real_frames(st, F)}
        rest = sorted(set(range(F)) - done)
        assert (_u16(prob)[rest] == PROB_CANARY).all()                 # a frame the launch does not address is not touched
    assert done == set(range(F))
    whole = _u16(buf)
    assert (whole[:pad] == PROB_CANARY).all() and (whole[pad + F * H * W:] == PROB_CANARY).all()
    got = _u16(prob).astype(np.float64)
    want, bound = ref.q_exact(merged, num), ref.q_bound(merged)
    assert (got[num == 0] == 0).all() and (got[np.isnan(merged)] == 0).all()
    for (y, x), (_val, q) in zip(spots, PLANTS):
        assert got[f0, y, x] == q, (y, x, _val, got[f0, y, x])
    if V > 1:
        f, y, x = planted["zero"]
        assert got[f, y, x] == 32768                                   # views holding x and -x: a merged +0.0
        f, y, x = planted["nan"]
        assert got[f, y, x] == 0                                       # +inf and -inf
    dist = np.abs(got - want)
    print("frame_probs F=%d %dx%d S=%d V=%d: max |q - 65535 sigmoid_f64| = %.4f LSB (bound at that pixel %.4f, smallest bound %.4f)"
          % (F, H, W, S, V, dist.max(), bound.reshape(-1)[dist.argmax()], bound.min()))
    assert (dist <= bound).all(), (float((dist - bound).max()), int(np.count_nonzero(dist > bound)))
    # a second run into a fresh map: the same bits; a fresh tensor from the call itself is zero where nothing was addressed
    again = torch.full_like(prob, PROB_CANARY)
    for x, st in zip(xd, launches):
        ops.frame_probs(x, views, st, F, H, W, prob=again)
    assert torch.equal(again, prob)
    fresh = ops.frame_probs(xd[0], views, launches[0], F, H, W)
    mine = sorted({f for _c, _k, f in real_frames(launches[0], F)})
    assert fresh.dtype == torch.int16 and torch.equal(fresh[mine], prob[mine]) and int(fresh.count_nonzero()) == int(prob[mine].count_nonzero())


def test_frame_probs_centre_crop_is_one_view_and_the_margin_is_zero():
    """The centre path of the engine: the one view (h0, w0, 0).  Inside the crop the value depends on the pixel's logit alone, so it equals
    a tiled run's value wherever only that view covers; the margin is 0 over the canary."""
    F, H, W, S, h0, w0 = 3, 9, 11, 4, 2, 3
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(1, 2, 8, S, S, generator=g) * 3).cuda()
    prob = torch.full((F, H, W), PROB_CANARY, dtype=torch.int16, device="cuda")
    ops.frame_probs(x, [(h0, w0, 0)], [0, 1], F, H, W, prob=prob)
    m = ref.Merge(F, H, W, S)
    m.add(x.cpu().numpy(), [(h0, w0, 0)], [0, 1])
    got = _u16(prob).astype(np.float64)
    inside = m.num > 0
    assert inside.sum() == F * S * S and (got[~inside] == 0).all() and (got[inside] > 0).any()
    assert (np.abs(got - ref.q_exact(m.merged(), m.num)) <= ref.q_bound(m.merged())).all()
    with pytest.raises(RuntimeError, match="view 0"):
        ops.frame_probs(x, [(H - S + 1, w0, 0)], [0, 1], F, H, W, prob=prob)
    with pytest.raises(ValueError, match="prob"):
        ops.frame_probs(x, [(h0, w0, 0)], [0, 1], F, H, W, prob=torch.zeros(F, H, W, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------- pc_instance_scores
def _check_scores(imap, prob, K, dev_imap=None, dev_prob=None):
    """imap uint8 / prob uint16 numpy [F,H,W] -> the restatement's (sums, npix); the kernel's record is exact against it, twice."""
    F = imap.shape[0]
    sums, npix = ref.slot_sums(imap, prob, K)
    di = torch.from_numpy(imap).cuda() if dev_imap is None else dev_imap
    dp = _dev16(prob) if dev_prob is None else dev_prob
    out = torch.full((F, 3 * (K + 1)), OUT_CANARY, dtype=torch.int32, device="cuda")
    assert ops.instance_scores(di, dp, K, out=out) is out
    got = out.cpu().numpy()
    assert np.array_equal(got, ref.words(sums, npix)), (got.tolist(), ref.words(sums, npix).tolist())
    s, n = ops.decode_instance_scores(got, K)
    assert np.array_equal(s, sums) and np.array_equal(n, npix)
    again = torch.full_like(out, OUT_CANARY)
    ops.instance_scores(di, dp, K, out=again)
    assert torch.equal(again, out)
    return sums, npix


def test_one_pixel_foreground_and_background():
    s, n = _check_scores(np.array([[[1]]], np.uint8), np.array([[[40000]]], np.uint16), K=1)
    assert s.tolist() == [[40000, 0]] and n.tolist() == [[1, 0]]
    s, n = _check_scores(np.array([[[0]]], np.uint8), np.array([[[40000]]], np.uint16), K=1)
    assert not s.any() and not n.any()
    s, n = _check_scores(np.array([[[2]]], np.uint8), np.array([[[65535]]], np.uint16), K=1)           # a value beyond K: the other slot
    assert s.tolist() == [[0, 65535]] and n.tolist() == [[0, 1]]


def _random_map(rng, shape, K, density=0.6):
    pool = np.array(list(range(1, K + 1)) + [255] + ([K + 1, 254, (K + 255) // 2] if K + 1 <= 254 else []), np.uint8)
    # runs of one value (a thread stays in a slot for a while) and single pixels (it changes slot at every pixel)
    imap = pool[rng.integers(0, pool.size, shape)]
    blocks = pool[rng.integers(0, pool.size, (shape[0], (shape[1] + 7) // 8, (shape[2] + 15) // 16))]
    coarse = np.repeat(np.repeat(blocks, 8, axis=1), 16, axis=2)[:, :shape[1], :shape[2]]
    imap = np.where(rng.random(shape) < 0.5, coarse, imap)
    return np.where(rng.random(shape) < density, imap, 0).astype(np.uint8)


def test_odd_addresses_of_both_inputs():
    F, H, W, K = 3, 9, 11, 4
    rng = np.random.default_rng(5)
    imap, prob = _random_map(rng, (F, H, W), K), rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    ibuf = torch.zeros(F * H * W + 7, dtype=torch.uint8, device="cuda")
    pbuf = torch.zeros(F * H * W + 7, dtype=torch.int16, device="cuda")
    di, dp = ibuf[1:1 + F * H * W].view(F, H, W), pbuf[1:1 + F * H * W].view(F, H, W)
    di.copy_(torch.from_numpy(imap)); dp.copy_(_dev16(prob))
    assert di.data_ptr() % 2 == 1 and (dp.data_ptr() // 2) % 2 == 1 and (H * W) % 2 == 1             # every frame of either at another alignment
    s, n = _check_scores(imap, prob, K, dev_imap=di, dev_prob=dp)
    assert n[:, :K].sum() > 0 and n[:, K].sum() > 0


@pytest.fixture(scope="module")
def random_inputs():
    rng = np.random.default_rng(29)
    return {K: _random_map(rng, (4, 37, 53), K) for K in (1, 8, 32)}, rng.integers(0, 65536, (4, 37, 53)).astype(np.uint16)


@pytest.mark.parametrize("K", (1, 8, 32))
def test_random_maps(random_inputs, K):
    maps, prob = random_inputs
    imap = maps[K]
    assert (imap == 255).any() and ((imap > K) & (imap < 255)).any() and all((imap == r + 1).any() for r in range(K))
    s, n = _check_scores(imap, prob, K)
    assert np.array_equal(n.sum(1), (imap != 0).reshape(4, -1).sum(1)) and n[:, K].min() > 0
    # whatever lies in prob under the background is not looked at
    other = prob.copy()
    other[imap == 0] = 0xFFFF
    s2, n2 = _check_scores(imap, other, K)
    assert np.array_equal(s, s2) and np.array_equal(n, n2)


def test_a_sub_range_writes_its_frames_and_nothing_else():
    F, H, W, K, pad = 4, 13, 17, 4, 64
    words = 3 * (K + 1)
    rng = np.random.default_rng(3)
    imap, prob = _random_map(rng, (F, H, W), K), rng.integers(0, 65536, (F, H, W)).astype(np.uint16)
    sums, npix = ref.slot_sums(imap, prob, K)
    obuf = torch.full((pad + F * words + pad,), OUT_CANARY, dtype=torch.int32, device="cuda")
    out = obuf[pad:pad + F * words].view(F, words)
    ops.instance_scores(torch.from_numpy(imap).cuda(), _dev16(prob), K, f0=1, nf=2, out=out)
    got, ob = out.cpu().numpy(), obuf.cpu().numpy()
    assert np.array_equal(got[1:3], ref.words(sums, npix)[1:3]) and (got[[0, 3]] == OUT_CANARY).all()
    assert (ob[:pad] == OUT_CANARY).all() and (ob[-pad:] == OUT_CANARY).all()
    with pytest.raises(RuntimeError, match="f0"):
        ops.instance_scores(torch.from_numpy(imap).cuda(), _dev16(prob), K, f0=3, nf=2, out=out)
    with pytest.raises(ValueError):
        ops.instance_scores(torch.from_numpy(imap).cuda(), _dev16(prob), 33)
    with pytest.raises(ValueError):
        ops.instance_scores(torch.from_numpy(imap).cuda(), _dev16(prob)[:2], K)


def test_a_sum_beyond_32_bits_sets_the_high_word():
    H, W = 257, 256
    s, n = _check_scores(np.ones((1, H, W), np.uint8), np.full((1, H, W), 65535, np.uint16), K=2)
    assert s[0].tolist() == [4311678720, 0, 0] and n[0].tolist() == [H * W, 0, 0] and 4311678720 > 2 ** 32
    out = ops.instance_scores(torch.ones(1, H, W, dtype=torch.uint8, device="cuda"), _dev16(np.full((1, H, W), 65535, np.uint16)), 2).cpu().numpy()
    assert out[0, :3].tolist() == [4311678720 - 2 ** 32, 1, H * W]
