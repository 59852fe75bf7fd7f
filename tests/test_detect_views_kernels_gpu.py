"""GPU: the two kernels of multi-view detection on their own (pc_clips_from_u8_views in csrc/evalclips.hip, pc_detect_frames_views in
csrc/detect.hip).

The cut kernel must write, per unflipped view, the bits pc_clips_from_u8 writes at that crop, per flipped view their left-right mirror image,
and nothing in front of, between (view_stride > n) or behind the views.  The two entries share a kernel, so every view is also held to the
numpy restatement of tests/clipcut_ref.py bit for bit.

The merge kernel is checked against the numpy float32 restatement of tests/detectviews_ref.py (views in table order, float32 adds, one
division): masks, counts and boxes exact; a frame score no further from float64 than the larger of 1e-6 and twice the distance of an fp32
torch evaluation (the rule of tests/test_detect_kernels_gpu.py: the factor two allows for another summation order).  Shapes: one view of one
frame (where mask, counts and boxes must also be pc_detect_frames'); 18 views of an odd-width frame with the mask at an odd address; 8 views
in two launches of three clips; one off-centre view and its mirror image under 32 clips in one launch, the uncovered margin written as 0
over a canary-filled mask.  A launch takes more clips than an F-frame video has by starts at or beyond F: those clips read and write nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, ops
from tests import clipcut_ref, detectviews_ref as ref

pytestmark = pytest.mark.gpu
SPECIALS = (0.0, -0.0, -5e-8, -1e-7, -9.9e-7, -1.1e-6, 80.0, -80.0, float("nan"))
MASK_CANARY, REC_CANARY, ROW0 = 0xAB, -77, 5


# ---------------------------------------------------------------------- pc_clips_from_u8_views
CUT_CASES = [  # F, H, W, S, views, starts, view_stride
    (3, 9, 11, 4, [(2, 3, 0), (2, 3, 1), (0, 0, 0), (5, 7, 1)], [0, 1], 2),
    (17, 10, 12, 8, [(1, 2, 0), (1, 2, 1)], [0, 1, 16], 5),
    (40, 12, 12, 8, [(3, 1, 0), (4, 4, 1)], list(range(32)), 35),      # 32 clips x 2 views in one launch; clips 26.. have frames beyond F
]


@pytest.mark.parametrize("F,H,W,S,views,starts,stride", CUT_CASES)
def test_clips_from_u8_views_writes_the_bits_of_clips_from_u8_per_view(F, H, W, S, views, starts, stride):
    g = torch.Generator().manual_seed(F + W)
    video = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    n, V, clip = len(starts), len(views), 32 * S * S
    assert stride >= n and V * n * 8 <= 8192
    body = ((V - 1) * stride + n) * clip
    buf = torch.full((64 + body + 64,), 7.0, device="cuda")
    out = ops.clips_from_u8_views(video, views, S, starts, view_stride=stride, out=buf[64:64 + body])
    assert out.data_ptr() == buf[64:].data_ptr()
    assert bool((buf[:64] == 7.0).all()) and bool((buf[64 + body:] == 7.0).all())
    slots = buf[64:64 + body].view(-1, 8, S, S, 4)
    host = clipcut_ref.cut(video.cpu().numpy(), views, S, starts)
    for v, (h0, w0, fl) in enumerate(views):
        want = ops.clips_from_u8(video, h0, w0, S, starts).view(n, 8, S, S, 4)
        if fl:
            want = want.flip(3)
        got = slots[v * stride:v * stride + n]
        assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (v, h0, w0, fl)      # the same bits
        assert clipcut_ref.same_bits(got, host[v]) and clipcut_ref.same_bits(want, host[v]), (v, h0, w0, fl)              # and the host's
        assert bool((got[..., 3] == 0).all())
        if v + 1 < V:
            assert bool((slots[v * stride + n:(v + 1) * stride] == 7.0).all()), v          # the stride gap is not written
    if stride == n:                                                      # the default stride, a fresh tensor
        fresh = ops.clips_from_u8_views(video, views, S, starts)
        assert fresh.shape == (V, n, 8, S, S, 4) and torch.equal(fresh.view(-1), buf[64:64 + body])
    if F == 40:
        past = [(c, k) for c, s in enumerate(starts) for k in range(8) if s + 2 * k >= F]
        assert past and all(bool((slots[v * stride + c, k] == 0).all()) for c, k in past for v in range(V))


# ---------------------------------------------------------------------- pc_detect_frames_views
def _covering(views, S, y, x):
    """[(view, row, column in the view's logits)] of the views that cover frame pixel (y, x), in table order."""
    out = []
    for v, (h0, w0, fl) in enumerate(views):
        if h0 <= y < h0 + S and w0 <= x < w0 + S:
            out.append((v, y - h0, S - 1 - (x - w0) if fl else x - w0))
    return out


def _logits(launches, views, F, H, W, S, seed):
    """Per launch float32 [V, n, 8, S, S]: normal noise times 3.  In the video's first real frame: the special values at the start of view 0
    and (where two or more views cover) one pixel whose views hold x, -x, x, -x .. (0.0 last for an odd number): a mean of exactly +0.0,
    positive; and one whose first two views hold +inf, -inf: NaN, background.  Then, as far as the video has frames for them: an all-negative
    frame, a full frame, and one frame with a single positive pixel at each corner of the covered region (the frame's, when tiled)."""
    g = torch.Generator().manual_seed(seed)
    V = len(views)
    xs = [(torch.randn(V, len(st), 8, S, S, generator=g) * 3).numpy() for st in launches]
    real = [(i, c, k, f) for i, st in enumerate(launches) for c, k, f in ref.real_frames(st, F)]
    cover = np.zeros((H, W), bool)
    for h0, w0, _fl in views:
        cover[h0:h0 + S, w0:w0 + S] = True
    ys, xs_ = np.nonzero(cover)
    ya, yb, xa, xb = ys.min(), ys.max(), xs_.min(), xs_.max()
    i, c, k, f = real[0]
    xs[i][0, c, k].reshape(-1)[:len(SPECIALS)] = SPECIALS
    planted = {}
    if V > 1:
        cov = _covering(views, S, yb, xb)
        assert len(cov) >= 2
        vals = [1.75 if j % 2 == 0 else -1.75 for j in range(len(cov))]
        if len(cov) % 2:
            vals[-1] = 0.0
        for (v, r, q), val in zip(cov, vals):
            xs[i][v, c, k, r, q] = val
        planted["zero"] = (f, yb, xb)
        cov = _covering(views, S, yb, xb - 1)
        assert len(cov) >= 2
        xs[i][cov[0][0], c, k, cov[0][1], cov[0][2]] = np.inf
        xs[i][cov[1][0], c, k, cov[1][1], cov[1][2]] = -np.inf
        planted["nan"] = (f, yb, xb - 1)
    plants = [("neg", None), ("pos", None)] + [("corner", yx) for yx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]
    for (kind, yx), (i, c, k, f) in zip(plants, real[1:]):
        x = xs[i]
        if kind == "pos":
            x[:, c, k] = np.abs(x[:, c, k])
        else:
            x[:, c, k] = -np.abs(x[:, c, k]) - 0.5
        if kind == "corner":
            for v, r, q in _covering(views, S, *yx):
                x[v, c, k, r, q] = 2.5
        planted.setdefault(kind, []).append((f, yx))
    return xs, planted, (ya, yb, xa, xb)


def _tiles(H, W, S):
    return detect.make_views(H, W, S, tile=True, flip=True)


MERGE_CASES = [  # F, H, W, S, views, bytes in front of the mask, launches (each: the starts of its clips; a start >= F: a clip without frames)
    (1, 4, 4, 4, [(0, 0, 0)], 16, ([0],)),
    (3, 9, 11, 4, _tiles(9, 11, 4), 13, ([0, 1],)),                                  # 18 views, odd W, the mask itself at an odd address
    (17, 10, 12, 8, _tiles(10, 12, 8), 16, ([0, 1, 17], [19, 16, 18])),              # 8 views, two launches of three clips
    (40, 12, 12, 8, [(3, 1, 0), (3, 1, 1)], 16, ([40 + c for c in range(13)] + [0, 1, 16] + [60 + c for c in range(13)] + [17, 32, 33],)),
]


@pytest.mark.parametrize("F,H,W,S,views,pad,launches", MERGE_CASES)
def test_detect_frames_views_against_a_numpy_restatement(F, H, W, S, views, pad, launches):
    V = len(views)
    assert sorted(s for st in launches for s in st if s < F) == evalstep.clip_starts(F, np.ones(F))     # the video's clips, each once
    assert {len(st) for st in launches} == {{1: 1, 3: 2, 17: 3, 40: 32}[F]} and V == {1: 1, 3: 18, 17: 8, 40: 2}[F]
    xs, planted, (ya, yb, xa, xb) = _logits(launches, views, F, H, W, S, seed=F * 100 + W)
    m = ref.Merge(F, H, W, S)
    for x, st in zip(xs, launches):
        m.add(x, views, st)
    merged, exp = m.merged(), m.masks()
    if V > 1:
        f, y, x = planted["zero"]
        assert merged[f, y, x] == 0.0 and not np.signbit(merged[f, y, x]) and exp[f, y, x] == 1
        f, y, x = planted["nan"]
        assert np.isnan(merged[f, y, x]) and exp[f, y, x] == 0
    mbuf = torch.full((pad + F * H * W + 16,), MASK_CANARY, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((8 + F * 8 + 8,), REC_CANARY, dtype=torch.int32, device="cuda")
    mask, rec = mbuf[pad:pad + F * H * W].view(F, H, W), rbuf[8:8 + F * 8].view(F, 8)
    assert mask.data_ptr() % 4 == pad % 4
    xd = [torch.from_numpy(x).cuda() for x in xs]
    done, first, row_of = set(), 0, {}
    for x, st in zip(xd, launches):
        ops.detect_frames_views(x, views, st, F, H, W, row0=ROW0 + first * V, mask=mask, rec=rec)
        for c, _k, f in ref.real_frames(st, F):
            row_of[f] = ROW0 + (first + c) * V
        done |= {f for _c, _k, f in ref.real_frames(st, F)}
        first += len(st)
        m_, r_ = mask.cpu().numpy(), rec.cpu().numpy()
        rest = sorted(set(range(F)) - done)
        assert (m_[rest] == MASK_CANARY).all() and (r_[rest] == REC_CANARY).all()            # a frame the launch does not address is not touched
    assert done == set(range(F))
    m_, r_ = mask.cpu().numpy(), rec.cpu().numpy()
    assert (mbuf[:pad].cpu() == MASK_CANARY).all() and (mbuf[pad + F * H * W:].cpu() == MASK_CANARY).all()
    assert (rbuf[:8].cpu() == REC_CANARY).all() and (rbuf[8 + F * 8:].cpu() == REC_CANARY).all()
    assert np.array_equal(m_, exp)                                                            # the uncovered margin included: 0 over the canary
    what = "detect_frames_views F=%d %dx%d S=%d V=%d" % (F, H, W, S, V)
    worst = worst32 = 0.0
    for f in range(F):
        cnt, x0, y0, x1, y1, bits, row, zero = (int(v) for v in r_[f])
        assert cnt == int(exp[f].sum()), (what, f, cnt, int(exp[f].sum()))
        assert (x0, y0, x1, y1) == ref.box_of(exp[f]), (what, f, (x0, y0, x1, y1), ref.box_of(exp[f]))
        assert row == row_of[f] and zero == 0
        score = float(np.array([bits], np.int32).view(np.float32)[0])
        if cnt == 0:
            assert bits == 0
            continue
        r64, r32 = ref.score_refs(merged[f], exp[f])
        d, d32 = abs(score - r64), abs(r32 - r64)
        worst, worst32 = max(worst, d), max(worst32, d32)
        assert d <= max(1e-6, 2.0 * d32), (what, f, score, r64, r32)
        assert 0.5 <= score <= 1.0
    print("%s: frame score |kernel-f64| %.3e  |fp32 torch-f64| %.3e" % (what, worst, worst32))
    if F >= 17:                                                       # the planted frames are there: empty, full, one pixel in each corner
        (fn, _), = planted["neg"]
        (fp, _), = planted["pos"]
        assert r_[fn, 0] == 0 and not r_[fn, 1:6].any()
        assert r_[fp, 0] == (yb - ya + 1) * (xb - xa + 1) and tuple(r_[fp, 1:5]) == (xa, ya, xb + 1, yb + 1)
        assert [tuple(r_[f, :5]) for f, _yx in planted["corner"]] == [(1, x_, y_, x_ + 1, y_ + 1) for _f, (y_, x_) in planted["corner"]]
        if len(views) == 8:
            assert (ya, yb, xa, xb) == (0, H - 1, 0, W - 1)          # tiled: the corners are the FRAME's
    if F == 1:                                                        # one unflipped view: the mask, counts and boxes of pc_detect_frames
        h0, w0, _fl = views[0]
        m1, r1 = ops.detect_frames(xd[0][0], launches[0], F, H, W, h0, w0, row0=ROW0)
        assert torch.equal(m1, mask) and torch.equal(r1[:, :5], rec[:, :5]) and torch.equal(r1[:, 6:], rec[:, 6:])
        s1 = float(r1[0, 5:6].cpu().numpy().view(np.float32)[0])
        r64, r32 = ref.score_refs(merged[0], exp[0])
        assert abs(s1 - r64) <= max(1e-6, 2.0 * abs(r32 - r64))
    # a second run gives the same records bit for bit; so does a run without masks
    for want_mask in (True, False):
        again = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
        first = 0
        for x, st in zip(xd, launches):
            m2, _r = ops.detect_frames_views(x, views, st, F, H, W, row0=ROW0 + first * V, rec=again, want_mask=want_mask)
            assert (m2 is None) == (not want_mask)
            first += len(st)
        assert torch.equal(again, rec), want_mask


def test_detect_frames_views_reads_its_views_at_the_callers_stride():
    """view_stride > n: the logits of view v of clip c at clip slot v * view_stride + c, NaN in the slots between."""
    F, H, W, S, views, st = 17, 10, 12, 8, _tiles(10, 12, 8), [0, 1, 16]
    (x,), _planted, _box = _logits((st,), views, F, H, W, S, seed=9)
    wide = np.full((len(views), 5, 8, S, S), np.nan, np.float32)
    wide[:, :3] = x
    want_m, want_r = ops.detect_frames_views(torch.from_numpy(x).cuda(), views, st, F, H, W, row0=ROW0)
    got_m, got_r = ops.detect_frames_views(torch.from_numpy(wide).cuda(), views, st, F, H, W, view_stride=5, row0=ROW0)
    assert torch.equal(got_m, want_m) and torch.equal(got_r, want_r) and int(want_r[:, 0].sum()) > 0
