"""GPU: pc_detect_frames_scaled (csrc/detectscale.hip) on its own, against the numpy float32 restatement of tests/resample_ref.py on top of
tests/detectviews_ref.Merge: the views merged on the working frame, the merged logits taken bilinearly to every native pixel, the cover
rule.  Masks, counts and boxes are exact; so is the probability map, whose expected value is pc_frame_probs' own conversion (the existing
entry, run on the RESTATED native logits laid out as one uncropped view) -- the header defines the map as that conversion of v.  A frame
score lies no further from float64 than the larger of 1e-6 and twice the distance of an fp32 torch evaluation, the bar of
tests/test_detect_views_kernels_gpu.py.

Shapes: the smallest at which each path of the two traversals is taken -- a down-sample onto an odd width, the identity (where every output
must be pc_detect_frames_views' and pc_frame_probs' bit for bit), an up-sample onto frames of odd H * W behind a mask and a probability map
at odd addresses, a centre crop that leaves most of the frame uncovered, a video in two launches, and a native frame of 1080 x 1920 at the
cap of 64 blocks per frame.  Every launch holds a clip whose later frames, or all of them, lie at or beyond F.  All buffers, the workspace
included, are filled with 0xa5 in front of the call."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, ops
from tests import resample_ref as ref

pytestmark = pytest.mark.gpu
ROW0, PAT = 5, 0xA5
REC_CANARY = int(np.array([PAT] * 4, np.uint8).view(np.int32)[0])
PROB_CANARY = int(np.array([PAT] * 2, np.uint8).view(np.uint16)[0])


def _tiles(H, W, S, flip):
    return detect.make_views(H, W, S, tile=True, flip=flip)


CASES = [  # F, Hs, Ws, S, H, W, views, bytes / elements in front of mask and prob, launches (a start >= F: a clip without frames)
    (3, 8, 8, 4, 5, 7, [(2, 3, 0), (2, 3, 1)], 16, ([0, 1, 3],)),                            # one view and its mirror image; down, odd W
    (2, 8, 12, 8, 8, 12, _tiles(8, 12, 8, False), 16, ([0, 1],)),                            # 2 tiles; the identity
    (9, 12, 12, 8, 31, 33, _tiles(12, 12, 8, True), 13, ([0, 1, 9],)),                       # 8 views; up, odd H * W, odd addresses
    (3, 40, 36, 16, 9, 10, [evalstep.centre_crop(40, 36, 16) + (0,)], 16, ([0, 1],)),        # centre crop: most of the frame uncovered; down
    (17, 120, 136, 112, 90, 160, _tiles(120, 136, 112, False), 16, ([0, 1, 17], [19, 16])),  # 4 tiles, two launches
    (1, 256, 256, 224, 1080, 1920, [evalstep.centre_crop(256, 256, 224) + (0,)], 16, ([0],)),      # 64 blocks per frame
]


def _covering(views, S, y, x):
    return [(v, y - h0, S - 1 - (x - w0) if fl else x - w0) for v, (h0, w0, fl) in enumerate(views) if h0 <= y < h0 + S and w0 <= x < w0 + S]


def _logits(launches, views, F, Hs, Ws, S, seed):
    """Per launch float32 [V, n, 8, S, S]: normal noise times 3 (normal range: no product with a weight >= 2^-12 is subnormal).  In the
    video's first real frame, at working pixels inside the first view: a 2 x 2 block whose every covering view holds +0.0 (merged +0.0 at two
    taps of a native pixel in each direction), one pixel of -0.0, one of NaN."""
    g = torch.Generator().manual_seed(seed)
    V = len(views)
    xs = [(torch.randn(V, len(st), 8, S, S, generator=g) * 3).numpy() for st in launches]
    i, (c, k, f) = next((i, r) for i, st in enumerate(launches) for r in ref.real_frames(st, F))
    h0, w0, _fl = views[0]
    planted = dict(frame=f, zero=[(h0 + 1, w0 + 1), (h0 + 1, w0 + 2), (h0 + 2, w0 + 1), (h0 + 2, w0 + 2)], negzero=(h0, w0 + 3), nan=(h0 + 3, w0))
    for (y, x), val in [(p, 0.0) for p in planted["zero"]] + [(planted["negzero"], -0.0), (planted["nan"], np.nan)]:
        for v, r, q in _covering(views, S, y, x):
            xs[i][v, c, k, r, q] = val
    return xs, planted


@pytest.mark.parametrize("F,Hs,Ws,S,H,W,views,pad,launches", CASES)
def test_detect_frames_scaled_against_a_numpy_restatement(F, Hs, Ws, S, H, W, views, pad, launches):
    V = len(views)
    assert sorted(s for st in launches for s in st if s < F) == evalstep.clip_starts(F, np.ones(F))     # the video's clips, each once
    assert any(s + 2 * k >= F for st in launches for s in st for k in range(8))                          # frames at or beyond F in the launches
    xs, planted = _logits(launches, views, F, Hs, Ws, S, seed=F * 100 + W)
    m = ref.Merge(F, Hs, Ws, S)
    for x, st in zip(xs, launches):
        m.add(x, views, st)
    merged = m.merged()
    f0 = planted["frame"]
    assert all(merged[f0, y, x] == 0.0 and not np.signbit(merged[f0, y, x]) for y, x in planted["zero"])
    assert np.signbit(merged[f0][planted["negzero"]]) and merged[f0][planted["negzero"]] == 0.0 and np.isnan(merged[f0][planted["nan"]])
    v, covered = ref.resample(merged, m.num, H, W)
    exp = ref.masks(v, covered)
    what = "detect_frames_scaled F=%d %dx%d -> %dx%d S=%d V=%d" % (F, Hs, Ws, H, W, S, V)
    print("%s: %d of %d native pixels covered, %d positive" % (what, int(covered.sum()), covered.size, int(exp.sum())))
    assert 0 < int(exp.sum()) < exp.size                                 # neither empty nor full: the comparison means something
    if len(views) == 1:
        assert 0 < int(covered.sum()) < covered.size                     # a centre crop: uncovered native pixels exist
    want_prob = ref.expected_probs(v, covered)
    assert not want_prob[~covered].any() and (want_prob[covered & ~np.isnan(v)] > 0).any()

    n_max = max(len(st) for st in launches)
    need = ops.detect_frames_scaled_ws_bytes(n_max, Hs, Ws, H, W)
    ws = torch.full((need,), PAT, dtype=torch.uint8, device="cuda")
    mbuf = torch.full((pad + F * H * W + 16,), PAT, dtype=torch.uint8, device="cuda")
    pbuf = torch.full((2 * (pad + F * H * W + 16),), PAT, dtype=torch.uint8, device="cuda").view(torch.int16)
    rbuf = torch.full((4 * (8 + F * 8 + 8),), PAT, dtype=torch.uint8, device="cuda").view(torch.int32)
    mask, prob, rec = mbuf[pad:pad + F * H * W].view(F, H, W), pbuf[pad:pad + F * H * W].view(F, H, W), rbuf[8:8 + F * 8].view(F, 8)
    assert mask.data_ptr() % 4 == pad % 4 and prob.data_ptr() % 8 == 2 * pad % 8
    xd = [torch.from_numpy(x).cuda() for x in xs]
    done, first, row_of = set(), 0, {}
    for x, st in zip(xd, launches):
        ws.fill_(PAT)
        ops.detect_frames_scaled(x, views, st, F, H, W, Hs, Ws, row0=ROW0 + first * V, mask=mask, prob=prob, rec=rec, ws=ws)
        for c, _k, f in ref.real_frames(st, F):
            row_of[f] = ROW0 + (first + c) * V
        done |= {f for _c, _k, f in ref.real_frames(st, F)}
        first += len(st)
        rest = sorted(set(range(F)) - done)
        if rest:                                                          # a frame the launch does not address keeps the canary
            assert (mask[rest].cpu().numpy() == PAT).all() and (rec[rest].cpu().numpy() == REC_CANARY).all()
            assert (prob[rest].cpu().numpy().view(np.uint16) == PROB_CANARY).all()
    assert done == set(range(F))
    m_, r_, p_ = mask.cpu().numpy(), rec.cpu().numpy(), prob.cpu().numpy().view(np.uint16)
    for buf, body in ((mbuf, F * H * W), (pbuf.view(torch.uint8), 2 * F * H * W)):
        lead = pad * buf.numel() // (pad + F * H * W + 16)
        b = buf.cpu().numpy()
        assert (b[:lead] == PAT).all() and (b[lead + body:] == PAT).all()
    assert (rbuf[:8].cpu().numpy() == REC_CANARY).all() and (rbuf[8 + F * 8:].cpu().numpy() == REC_CANARY).all()
    assert np.array_equal(m_, exp)                                        # the uncovered pixels included: 0 over the canary
    assert np.array_equal(p_, want_prob)
    worst = worst32 = 0.0
    for f in range(F):
        cnt, x0, y0, x1, y1, bits, row, zero = (int(t) for t in r_[f])
        assert cnt == int(exp[f].sum()), (what, f, cnt, int(exp[f].sum()))
        assert (x0, y0, x1, y1) == ref.box_of(exp[f]), (what, f, (x0, y0, x1, y1), ref.box_of(exp[f]))
        assert row == row_of[f] and zero == 0
        score = float(np.array([bits], np.int32).view(np.float32)[0])
        if cnt == 0:
            assert bits == 0
            continue
        r64, r32 = ref.score_refs(v[f], exp[f])
        d, d32 = abs(score - r64), abs(r32 - r64)
        worst, worst32 = max(worst, d), max(worst32, d32)
        assert d <= max(1e-6, 2.0 * d32), (what, f, score, r64, r32)
    print("%s: frame score |kernel-f64| %.3e  |fp32 torch-f64| %.3e" % (what, worst, worst32))
    if (Hs, Ws) == (H, W):                                               # the identity: pc_detect_frames_views and pc_frame_probs, bit for bit
        assert np.array_equal(v.view(np.int32), merged.view(np.int32)) and np.array_equal(covered, m.num >= 1)
        m1 = torch.full((F, H, W), PAT, dtype=torch.uint8, device="cuda")
        r1 = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
        p1 = torch.full((F, H, W), 0, dtype=torch.int16, device="cuda")
        first = 0
        for x, st in zip(xd, launches):
            ops.detect_frames_views(x, views, st, F, H, W, row0=ROW0 + first * V, mask=m1, rec=r1)
            ops.frame_probs(x, views, st, F, H, W, prob=p1)
            first += len(st)
        assert torch.equal(m1, mask) and torch.equal(r1, rec) and torch.equal(p1, prob)
    # a second run gives the same records bit for bit; so does a run without mask, without prob, without either
    for want_mask, want_prob_ in ((True, True), (False, True), (True, False), (False, False)):
        again = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
        p2 = torch.full((F, H, W), 0, dtype=torch.int16, device="cuda") if want_prob_ else None
        first = 0
        for x, st in zip(xd, launches):
            m2, _r = ops.detect_frames_scaled(x, views, st, F, H, W, Hs, Ws, row0=ROW0 + first * V, prob=p2, rec=again, want_mask=want_mask)
            assert (m2 is None) == (not want_mask)
            first += len(st)
        assert torch.equal(again, rec), (want_mask, want_prob_)
        assert p2 is None or torch.equal(p2, prob)


def test_detect_frames_scaled_reads_its_views_at_the_callers_stride():
    F, Hs, Ws, S, H, W, views, st = 17, 12, 12, 8, 10, 9, _tiles(12, 12, 8, True), [0, 1, 16]
    (x,), _planted = _logits((st,), views, F, Hs, Ws, S, seed=9)
    wide = np.full((len(views), 5, 8, S, S), np.nan, np.float32)
    wide[:, :3] = x
    p1, p2 = (torch.zeros(F, H, W, dtype=torch.int16, device="cuda") for _ in range(2))
    want_m, want_r = ops.detect_frames_scaled(torch.from_numpy(x).cuda(), views, st, F, H, W, Hs, Ws, row0=ROW0, prob=p1)
    got_m, got_r = ops.detect_frames_scaled(torch.from_numpy(wide).cuda(), views, st, F, H, W, Hs, Ws, view_stride=5, row0=ROW0, prob=p2)
    assert torch.equal(got_m, want_m) and torch.equal(got_r, want_r) and torch.equal(p1, p2) and int(want_r[:, 0].sum()) > 0


def test_the_ops_refuse_bad_arguments():
    F, Hs, Ws, S, H, W, views, st = 3, 8, 8, 4, 5, 7, [(2, 3, 0), (2, 3, 1)], [0, 1]
    x = torch.zeros(2, 2, 8, S, S, device="cuda")
    tab = ops.resample_tables(Hs, Ws, H, W, "cuda")
    assert tab.dtype == torch.int32 and tab.numel() == 2 * (H + W) and tab is ops.resample_tables(Hs, Ws, H, W, "cuda")      # cached
    assert np.array_equal(tab.cpu().numpy(), ref.tables(Hs, Ws, H, W))
    assert ops.detect_frames_scaled_ws_bytes(2, Hs, Ws, H, W) == ops.detect_frames_views_ws_bytes(2, H, W) + 16 + 2 * 8 * 64 * 5
    good = dict(logits=x, views=views, starts=st, F=F, H=H, W=W, Hs=Hs, Ws=Ws)
    ops.detect_frames_scaled(**good)
    bad = [dict(logits=x.double()), dict(logits=x[..., :3]), dict(logits=x[:1]), dict(view_stride=1), dict(views=[(0, 0)]), dict(views=[]),
           dict(H=0), dict(W=1 << 23), dict(mask=torch.zeros(F, H, W + 1, dtype=torch.uint8, device="cuda")),
           dict(mask=torch.zeros(F, H, W, dtype=torch.int32, device="cuda")), dict(prob=torch.zeros(F, H, W, dtype=torch.float32, device="cuda")),
           dict(prob=torch.zeros(F, H, W + 1, dtype=torch.int16, device="cuda")), dict(rec=torch.zeros(F, 7, dtype=torch.int32, device="cuda")),
           dict(ws=torch.zeros(ops.detect_frames_scaled_ws_bytes(2, Hs, Ws, H, W) - 1, dtype=torch.uint8, device="cuda")),
           dict(mask=torch.zeros(F, H, W, dtype=torch.uint8))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.detect_frames_scaled(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="pc_detect_frames_scaled"):         # what the wrapper leaves to the library: a view outside the WORKING frame
        ops.detect_frames_scaled(**dict(good, views=[(5, 3, 0)]))
    with pytest.raises(RuntimeError, match="pc_resample_tables"):
        ops.resample_tables(8, 8, 0, 4, "cuda")
