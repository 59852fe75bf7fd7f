"""GPU: the kernels of the detection output (csrc/detect.hip, and the truth switch of csrc/evalclips.hip) on their own.

pc_clips_from_u8 must write the bits pc_eval_clips_from_u8 writes, and both (one kernel) those of the numpy restatement of
tests/clipcut_ref.py, truth included.  pc_detect_frames is checked against a torch restatement (sigmoid >= 0.5,
the clip interleave undone on the host, pasted into full frames) at the smallest shapes at which each of its parts can go wrong: a clip with
seven frames past the end; an odd W and a mask that starts at an odd address (byte stores); three clips whose frames interleave; two launches
into one video; 32 clips in one launch; and one frame whose mask lies beyond byte 2^31.  Masks, counts and boxes are exact; the count also
equals what pc_seg_frame_counts gives for the same logits (the shared predicate, tie band included); a frame score may be no further from
float64 than the larger of 1e-6 and twice the distance of an fp32 torch evaluation (the rule of tests/test_valmetrics_gpu.py: the factor two
allows for another summation order).  pc_video_class against evalstep.vote, numpy and pc_video_vote."""
import numpy as np
import pytest
import torch

from picons_amd import evalstep, ops
from tests import clipcut_ref

pytestmark = pytest.mark.gpu
SPECIALS = (0.0, -0.0, -5e-8, -1e-7, -9.9e-7, -1.1e-6, 80.0, -80.0, float("inf"), float("-inf"), float("nan"))
MASK_CANARY, REC_CANARY, ROW0 = 0xAB, -77, 5


def _real_frames(starts, F):
    return [(c, k, s + 2 * k) for c, s in enumerate(starts) for k in range(8) if s + 2 * k < F]


def _logits(starts, F, S, seed):
    """Normal noise times 3 with the special values in the first real frame and, as far as the video has frames for them, an all-negative
    frame, a full-positive frame and one frame with a single positive pixel at each crop corner."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(len(starts), 8, S, S, generator=g) * 3
    real = _real_frames(starts, F)
    c, k, _f = real[0]
    x[c, k].view(-1)[:len(SPECIALS)] = torch.tensor(SPECIALS)
    plants = [("neg", None), ("pos", None)] + [("corner", yx) for yx in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1))]
    for (kind, yx), (c, k, _f) in zip(plants, real[1:]):
        if kind == "neg":
            x[c, k] = -x[c, k].abs() - 0.5
        elif kind == "pos":
            x[c, k] = x[c, k].abs()
        else:
            x[c, k] = -x[c, k].abs() - 0.5
            x[c, k, yx[0], yx[1]] = 2.5
    return x


def _expected(x, starts, F, H, W, S, h0, w0):
    pos = torch.sigmoid(x) >= 0.5                                   # the evaluator's predicate as the reference states it, fp32 on the host
    mask = np.zeros((F, H, W), np.uint8)
    for c, k, f in _real_frames(starts, F):
        mask[f, h0:h0 + S, w0:w0 + S] = pos[c, k].numpy()
    return mask


def _check_frames(x, starts, frames, mask, rec, exp, S, h0, w0, what):
    """Records (and masks, if given) of the video frames `frames` against the expected masks; -> the two largest score distances."""
    union = ops.seg_frame_counts(x.cuda(), torch.zeros_like(x).cuda()).cpu().numpy()[:, 1].reshape(len(starts), 8)
    where = {f: (c, k) for c, k, f in _real_frames(starts, exp.shape[0])}
    worst = worst32 = 0.0
    for f in frames:
        c, k = where[f]
        if mask is not None:
            assert np.array_equal(mask[f], exp[f]), (what, f)
        cnt, x0, y0, x1, y1, bits, row, zero = (int(v) for v in rec[f])
        assert cnt == int(exp[f].sum()) == int(union[c, k]), (what, f, cnt, int(exp[f].sum()), int(union[c, k]))
        ys, xs = np.nonzero(exp[f])
        box = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if cnt else (0, 0, 0, 0)
        assert (x0, y0, x1, y1) == box, (what, f, (x0, y0, x1, y1), box)
        assert int(exp[f, y0:y1, x0:x1].sum()) == cnt
        assert row == ROW0 + c and zero == 0
        score = float(np.array([bits], np.int32).view(np.float32)[0])
        if cnt == 0:
            assert bits == 0
            continue
        sel = x[c, k][torch.from_numpy(exp[f, h0:h0 + S, w0:w0 + S].astype(bool))]          # the kernel's own positive set
        ref = float((1.0 / (1.0 + torch.exp(-sel.double()))).mean())
        f32 = float((1.0 / (1.0 + torch.exp(-sel))).mean())
        d, d32 = abs(score - ref), abs(f32 - ref)
        worst, worst32 = max(worst, d), max(worst32, d32)
        assert d <= max(1e-6, 2.0 * d32), (what, f, score, ref, f32)
        assert 0.5 <= score <= 1.0
    return worst, worst32


CASES = [  # F, H, W, S, h0, w0, bytes in front of the mask, launches (each: how many of the video's clips)
    (1, 4, 4, 4, 0, 0, 16, (1,)),             # seven of the clip's eight frames lie beyond F
    (3, 9, 11, 4, 2, 3, 13, (2,)),            # odd W, the mask itself at an odd address: unaligned rows
    (17, 10, 12, 8, 1, 2, 16, (3,)),          # starts 0, 1, 16
    (40, 12, 12, 8, 0, 0, 16, (3, 3)),        # six clips as two launches of three
    (256, 8, 8, 8, 0, 0, 16, (32,)),          # 32 clips in one launch
]


@pytest.mark.parametrize("F,H,W,S,h0,w0,pad,launches", CASES)
def test_detect_frames_against_a_torch_restatement(F, H, W, S, h0, w0, pad, launches):
    starts = evalstep.clip_starts(F, np.ones(F))
    assert len(starts) == sum(launches)
    x = _logits(starts, F, S, seed=F * 100 + W)
    exp = _expected(x, starts, F, H, W, S, h0, w0)
    xd = x.cuda()
    mbuf = torch.full((pad + F * H * W + 16,), MASK_CANARY, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((8 + F * 8 + 8,), REC_CANARY, dtype=torch.int32, device="cuda")
    mask, rec = mbuf[pad:pad + F * H * W].view(F, H, W), rbuf[8:8 + F * 8].view(F, 8)
    assert mask.data_ptr() % 4 == pad % 4
    done, first = set(), 0
    for n in launches:
        seg = starts[first:first + n]
        ops.detect_frames(xd[first:first + n], seg, F, H, W, h0, w0, row0=ROW0 + first, mask=mask, rec=rec)
        done |= {f for _c, _k, f in _real_frames(seg, F)}
        first += n
        m_, r_ = mask.cpu().numpy(), rec.cpu().numpy()
        rest = sorted(set(range(F)) - done)
        assert (m_[rest] == MASK_CANARY).all() and (r_[rest] == REC_CANARY).all()            # a frame the launch does not address is not touched
    assert done == set(range(F))
    m_, r_ = mask.cpu().numpy(), rec.cpu().numpy()
    assert (mbuf[:pad].cpu() == MASK_CANARY).all() and (mbuf[pad + F * H * W:].cpu() == MASK_CANARY).all()
    assert (rbuf[:8].cpu() == REC_CANARY).all() and (rbuf[8 + F * 8:].cpu() == REC_CANARY).all()
    assert set(np.unique(m_).tolist()) <= {0, 1}
    what = "detect_frames F=%d %dx%d S=%d" % (F, H, W, S)
    d, d32 = _check_frames(x, starts, range(F), m_, r_, exp, S, h0, w0, what)
    print("%s: frame score |kernel-f64| %.3e  |fp32 torch-f64| %.3e" % (what, d, d32))
    if F >= 17:                                                       # the planted frames are there: empty, full, one pixel in each corner
        fr = [f for _c, _k, f in _real_frames(starts, F)][1:7]
        assert r_[fr[0], 0] == 0 and not r_[fr[0], 1:6].any() and r_[fr[1], 0] == S * S
        assert [tuple(r_[f, :5]) for f in fr[2:]] == [(1, w0 + x_, h0 + y_, w0 + x_ + 1, h0 + y_ + 1) for y_, x_ in
                                                      ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1))]
    # a second run gives the same records bit for bit; so does a run without masks
    for want_mask in (True, False):
        again = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
        first = 0
        for n in launches:
            m2, _r = ops.detect_frames(xd[first:first + n], starts[first:first + n], F, H, W, h0, w0, row0=ROW0 + first, rec=again, want_mask=want_mask)
            assert (m2 is None) == (not want_mask)
            first += n
        assert torch.equal(again, rec), want_mask


def test_detect_frames_beyond_byte_2_to_the_31():
    """A video of 2100 frames of 1024 x 1024: the last clip's masks lie more than 2^31 bytes into the buffer.  Only the frames the launch
    addresses are written, so only they and their neighbours are looked at."""
    F, H, W, S, h0, w0 = 2100, 1024, 1024, 8, 500, 508
    starts = [2090]                                                   # frames 2090, 2092 .. 2098; 2100 .. 2104 lie beyond F
    x = _logits(starts, F, S, seed=3)
    mask = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    for f in (2089, 2091, 2097, 2099):
        mask[f].fill_(MASK_CANARY)
    rec = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
    ops.detect_frames(x.cuda(), starts, F, H, W, h0, w0, row0=ROW0, mask=mask, rec=rec)
    assert 2098 * H * W > 2 ** 31
    pos = (torch.sigmoid(x) >= 0.5).numpy()
    r_ = rec.cpu().numpy()
    for k, f in enumerate(range(2090, 2100, 2)):
        exp = np.zeros((H, W), np.uint8)
        exp[h0:h0 + S, w0:w0 + S] = pos[0, k]
        assert np.array_equal(mask[f].cpu().numpy(), exp), f
        ys, xs = np.nonzero(exp)
        assert r_[f, 0] == exp.sum() and (r_[f, 0] == 0 or tuple(r_[f, 1:5]) == (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1))
    for f in (2089, 2091, 2097, 2099):
        assert bool((mask[f] == MASK_CANARY).all()) and (r_[f] == REC_CANARY).all()
    assert (r_[:2090] == REC_CANARY).all()


@pytest.mark.parametrize("F,H,W,S,h0,w0", [(1, 8, 8, 8, 0, 0), (3, 9, 11, 4, 2, 3), (17, 10, 12, 8, 1, 2)])
def test_clips_from_u8_writes_the_bits_of_eval_clips_from_u8(F, H, W, S, h0, w0):
    g = torch.Generator().manual_seed(F + W)
    video = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    truth = torch.randint(0, 3, (F, H, W), generator=g, dtype=torch.uint8).cuda()
    starts = evalstep.clip_starts(F, np.ones(F))
    n = len(starts)
    want, gt = ops.eval_clips_from_u8(video, truth, h0, w0, S, starts)
    ref_data, ref_gt = clipcut_ref.cut(video.cpu().numpy(), [(h0, w0, 0)], S, starts, truth=truth.cpu().numpy())
    assert clipcut_ref.same_bits(want, ref_data) and clipcut_ref.same_bits(gt, ref_gt)              # both entries share a kernel: the host's bits
    buf = torch.full((64 + n * 32 * S * S + 64,), 7.0, device="cuda")
    got = ops.clips_from_u8(video, h0, w0, S, starts, out=buf[64:64 + n * 32 * S * S])
    assert torch.equal(got.view(-1).view(torch.int32), want.view(-1).view(torch.int32))            # the same bits, -0.0 and all
    assert clipcut_ref.same_bits(got, ref_data)
    assert bool((buf[:64] == 7.0).all()) and bool((buf[64 + n * 32 * S * S:] == 7.0).all())
    assert torch.equal(ops.clips_from_u8(video, h0, w0, S, starts).view(-1), want.view(-1))
    assert bool((want.view(n, 8, S, S, 4)[..., 3] == 0).all()) and (F >= 16 or bool((want.view(n, 8, S, S, 4)[0, 7] == 0).all()))


def _mean_rows(p):
    s = p[0].copy()
    for r in p[1:]:
        s = (s + r).astype(np.float32)
    return (s / np.float32(p.shape[0])).astype(np.float32)


@pytest.mark.parametrize("n", (1, 3, 32))
@pytest.mark.parametrize("C", (21, 24))
def test_video_class_against_vote_numpy_and_video_vote(n, C):
    rng = np.random.default_rng(n * 100 + C)
    plain = rng.standard_normal((n, C)).astype(np.float32)
    tie = plain.copy()
    tie[:, 5] = np.abs(plain).max() + 1; tie[:, 17] = tie[:, 5]                  # an exact tie: the first maximum wins
    nan = tie.copy()
    nan[n // 2, 9] = np.nan                                                       # a NaN column beats every number
    both = nan.copy()
    both[0, 3] = np.nan                                                           # two of them: the first
    for name, p, want in (("plain", plain, None), ("tie", tie, 5), ("nan", nan, 9), ("two nans", both, 3)):
        dev = torch.from_numpy(p).cuda()
        out = ops.video_class(dev).cpu().numpy()
        means = _mean_rows(p)
        assert out.shape == (C + 2,) and np.array_equal(out[:C].view(np.int32), means.view(np.int32)), name
        best = evalstep.vote(p)
        assert best == int(np.argmax(np.mean(p, axis=0))) and (want is None or best == want), name
        assert out[C] == float(best), (name, out[C], best)
        assert np.array_equal(out[C + 1:].view(np.int32), means[best:best + 1].view(np.int32)), name
        hits = torch.zeros(1, dtype=torch.int32, device="cuda")                   # what pc_video_vote counts as correct is that arg-max
        ops.video_vote(dev, best, hits)
        ops.video_vote(dev, (best + 1) % C, hits)
        assert int(hits) == 1, name
