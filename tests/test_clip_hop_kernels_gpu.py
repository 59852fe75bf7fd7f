"""GPU: pc_clip_planes and pc_detect_frames_planes (csrc/cliphop.hip) on their own, against a numpy restatement: tests/detectviews_ref.Merge per
clip gives each slot plane and the cover bytes, the float32 mean over the windows that hold a frame is written one operation at a time in
window order (the first value as it is, the others added, one division by the count when it is above 1), and from there
tests/resample_ref.py: resample, masks, box_of, score_refs, and expected_probs for the probability.  Planes, cover bytes, masks, counts,
boxes, probabilities and record words 6 and 7 are exact; a frame score lies no further from float64 than the larger of 1e-6 and twice the
distance of an fp32 torch evaluation, the bar of tests/test_detect_scaled_kernels_gpu.py.

Every output buffer stands between 0xa5 canaries, the planes are filled with NaN in front of the first launch -- a (slot, frame) no clip
addressed must still hold it, and a read of one would show in every output --, and the logits are 3 x normal noise with the special values
of tests/test_detect_kernels_gpu.py, an all-negative and a full frame planted in every clip that holds the frame."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, ops
from tests import clip_hop_ref as hop_ref, resample_ref as ref

pytestmark = pytest.mark.gpu
ROW0, PAT = 5, 0xA5
REC_CANARY = int(np.array([PAT] * 4, np.uint8).view(np.int32)[0])
PROB_CANARY = int(np.array([PAT] * 2, np.uint8).view(np.uint16)[0])
SPECIALS = (0.0, -0.0, -5e-8, -1e-7, -9.9e-7, -1.1e-6, 80.0, -80.0, float("inf"), float("-inf"), float("nan"))
NAN_BITS = int(np.array([np.nan], np.float32).view(np.int32)[0])
S = 8
CENTRE = [evalstep.centre_crop(10, 12, S) + (0,)]
MIRRORED = [(0, 0, 0), (0, 0, 1), (2, 5, 0), (2, 5, 1)]
TWO = [(0, 0, 0), (4, 8, 1)]                                           # of a 12 x 16 frame: a corner each, the other two uncovered

CASES = [  # name, F, f_skip, hop, Hs, Ws, H, W, views, bytes / elements in front of mask and prob
    ("a", 17, 2, 8, 10, 12, 10, 12, CENTRE, 16),                       # cover 1, 2, 1; the last frame is held by one window
    ("b6", 40, 2, 6, 10, 12, 10, 12, CENTRE, 16),                      # M = 3, the hop does not divide the span
    ("b2", 40, 2, 2, 10, 12, 10, 12, CENTRE, 16),                      # M = 8
    ("c", 33, 2, 4, 10, 13, 10, 13, MIRRORED, 13),                     # odd width, mask and prob at odd addresses, pstride 132 > 130
    ("d-down", 33, 2, 8, 12, 16, 9, 11, TWO, 16),
    ("d-up", 33, 2, 8, 12, 16, 20, 27, TWO, 13),
    ("e1", 20, 1, 1, 10, 12, 10, 12, CENTRE, 16),
    ("e3", 20, 3, 3, 10, 12, 10, 12, CENTRE, 16),
]


_ceil, _holders = hop_ref.ceil_div, hop_ref.holders


def _logits(starts, F, fs, hop, views, seed):
    """float32 [V, n, 8, S, S].  Frame 0 of the video: the special values at frame pixels of the first view, in every view that covers the
    pixel; the video's middle frame all negative and the one behind it all positive, in every clip that holds them."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(len(views), len(starts), 8, S, S, generator=g) * 3).numpy()
    h0, w0, _fl = views[0]
    for c, k in _holders(starts, F, fs, hop, 0):
        for i, val in enumerate(SPECIALS):
            y, xx = h0 + i // 4, w0 + i % 4
            for v, (vh, vw, fl) in enumerate(views):
                if vh <= y < vh + S and vw <= xx < vw + S:
                    x[v, c, k, y - vh, S - 1 - (xx - vw) if fl else xx - vw] = val
    for f, sign in ((F // 2, -1.0), (F // 2 + 1, 1.0)):
        for c, k in _holders(starts, F, fs, hop, f):
            x[:, c, k] = sign * (np.abs(x[:, c, k]) + 0.5)
    return x


def _restate(x, starts, F, fs, hop, views, Hs, Ws):
    return hop_ref.restate(x, starts, F, fs, hop, views, Hs, Ws, S)


class Buffers:
    """The planes filled with NaN and every output between 0xa5 canaries."""

    def __init__(self, F, fs, hop, Hs, Ws, H, W, pad):
        self.F, self.H, self.W, self.pad = F, H, W, pad
        self.need = ops.clip_planes_bytes(F, Hs, Ws, fs, hop)
        self.ps = (Hs * Ws + 3) // 4 * 4
        self.pbuf = torch.full((16 + self.need + 16,), PAT, dtype=torch.uint8, device="cuda")
        self.planes = self.pbuf[16:16 + self.need]
        self.plane, self.cover = ops.clip_plane_views(self.planes, F, Hs, Ws, fs, hop)
        self.plane.fill_(float("nan"))
        assert self.plane.shape == (_ceil(8 * fs, hop), F, self.ps) and self.cover.shape == (self.ps,)
        n = F * H * W
        self.mbuf = torch.full((pad + n + 16,), PAT, dtype=torch.uint8, device="cuda")
        self.qbuf = torch.full((2 * (pad + n + 16),), PAT, dtype=torch.uint8, device="cuda").view(torch.int16)
        self.rbuf = torch.full((4 * (8 + F * 8 + 8),), PAT, dtype=torch.uint8, device="cuda").view(torch.int32)
        self.mask, self.prob, self.rec = self.mbuf[pad:pad + n].view(F, H, W), self.qbuf[pad:pad + n].view(F, H, W), self.rbuf[8:8 + F * 8].view(F, 8)
        self.ws = torch.full((ops.detect_frames_planes_ws_bytes(min(F, ops.PLANES_MAX_FRAMES), H, W) + 16,), PAT, dtype=torch.uint8, device="cuda")

    def canaries_intact(self):
        p = self.pbuf.cpu().numpy()
        assert (p[:16] == PAT).all() and (p[16 + self.need:] == PAT).all()
        n = self.F * self.H * self.W
        for buf, lead, body in ((self.mbuf, self.pad, n), (self.qbuf.view(torch.uint8), 2 * self.pad, 2 * n)):
            b = buf.cpu().numpy()
            assert (b[:lead] == PAT).all() and (b[lead + body:] == PAT).all()
        assert (self.rbuf[:8].cpu().numpy() == REC_CANARY).all() and (self.rbuf[8 + self.F * 8:].cpu().numpy() == REC_CANARY).all()
        assert (self.ws[-16:].cpu().numpy() == PAT).all()

    def outputs(self):
        return self.mask.cpu().numpy(), self.rec.cpu().numpy(), self.prob.cpu().numpy().view(np.uint16)


def _fill_planes(b, x, starts, F, fs, hop, views, Hs, Ws, launches):
    """The clips of `launches` (lists of clip indices) through pc_clip_planes, the cover with the first launch."""
    for i, idx in enumerate(launches):
        ops.clip_planes(torch.from_numpy(np.ascontiguousarray(x[:, idx])).cuda(), views, [starts[c] for c in idx], F, Hs, Ws, fs, hop, planes=b.planes,
                        cover=i == 0)


def _detect(b, F, H, W, Hs, Ws, V, fs, hop, ranges, mask=True, prob=True, rec=None):
    for f0, nf in ranges:
        ops.detect_frames_planes(b.planes, F, H, W, Hs, Ws, V, fs, hop, f0, nf, row0=ROW0, mask=b.mask if mask else None, prob=b.prob if prob else None,
                                 rec=b.rec if rec is None else rec, ws=b.ws[:-16], want_mask=False)


def _check_planes(b, per, num, starts, F, fs, hop, Hs, Ws):
    """Every addressed (slot, frame) holds the clip's merged logits bit for bit, zeros in its padding; every other one still the NaN it was
    filled with; the cover bytes are the counts, zeros in the padding."""
    M = _ceil(8 * fs, hop)
    got = b.plane.cpu().numpy().view(np.int32)
    want = np.full((M, F, b.ps), NAN_BITS, np.int32)
    for c, s in enumerate(starts):
        for k in range(8):
            if s + k * fs < F:
                slot = want[(s // hop) % M, s + k * fs]
                assert (slot == NAN_BITS).all()                           # no two clips share a (slot, frame)
                slot[:] = 0
                slot[:Hs * Ws] = per[c, k].reshape(-1).view(np.int32)
    for a in (got, want):                                               # a NaN is a NaN: which payload an addition hands on is the machine's
        a[np.isnan(a.view(np.float32))] = NAN_BITS
    assert np.array_equal(got, want)
    cov = np.zeros(b.ps, np.uint8)
    cov[:Hs * Ws] = num.reshape(-1)
    assert np.array_equal(b.cover.cpu().numpy(), cov)


def _setup(F, fs, hop, Hs, Ws, views, seed):
    starts = detect.clip_starts_hop(F, fs, hop)
    assert starts == ops.clip_hop_starts(F, fs, hop) and len(starts) <= 32
    x = _logits(starts, F, fs, hop, views, seed)
    return (starts, x) + _restate(x, starts, F, fs, hop, views, Hs, Ws)


@pytest.mark.parametrize("name,F,fs,hop,Hs,Ws,H,W,views,pad", CASES, ids=[c[0] for c in CASES])
def test_planes_and_frames_against_a_numpy_restatement(name, F, fs, hop, Hs, Ws, H, W, views, pad):
    V = len(views)
    starts, x, per, num, mean = _setup(F, fs, hop, Hs, Ws, views, seed=F * 100 + W + hop)
    covers = [len(_holders(starts, F, fs, hop, f)) for f in range(F)]
    if name == "a":
        assert covers == [1] * 8 + [2] * 8 + [1] and _holders(starts, F, fs, hop, 16) == [(2, 4)]
    if name in ("b6", "b2", "c", "e1"):
        assert max(covers) == _ceil(8 * fs, hop) and min(covers) == 1
    v, covered = ref.resample(mean, np.broadcast_to(num, mean.shape), H, W)
    exp = ref.masks(v, covered)
    what = "clip hop %s F=%d f_skip=%d hop=%d %dx%d -> %dx%d V=%d" % (name, F, fs, hop, Hs, Ws, H, W, V)
    print("%s: %d clips, cover %d..%d, %d of %d native pixels covered, %d positive" % (what, len(starts), min(covers), max(covers), int(covered.sum()),
                                                                                          covered.size, int(exp.sum())))
    assert 0 < int(exp.sum()) < exp.size and 0 < int(covered.sum()) < covered.size
    assert not exp[F // 2].any() and np.array_equal(exp[F // 2 + 1], covered[F // 2 + 1].astype(np.uint8))      # the all-negative and the full frame
    if (Hs, Ws) == (H, W) and V == 1:                                   # the special values reach the merged logit of frame 0
        h0, w0, _fl = views[0]
        head = mean[0, h0:h0 + 3, w0:w0 + 4].reshape(-1)[:len(SPECIALS)]
        assert np.isnan(head[10]) and np.isinf(head[8]) and np.isinf(head[9]) and np.signbit(head[1]) and head[1] == 0.0 and not np.signbit(head[0])
    want_prob = ref.expected_probs(v, covered)
    assert not want_prob[~covered].any() and (want_prob[covered & ~np.isnan(v)] > 0).any()

    b = Buffers(F, fs, hop, Hs, Ws, H, W, pad)
    assert b.mask.data_ptr() % 4 == pad % 4 and b.prob.data_ptr() % 8 == 2 * pad % 8
    _fill_planes(b, x, starts, F, fs, hop, views, Hs, Ws, [list(range(len(starts)))])
    _check_planes(b, per, num, starts, F, fs, hop, Hs, Ws)
    _detect(b, F, H, W, Hs, Ws, V, fs, hop, [(0, F // 2), (F // 2, F - F // 2)])
    b.canaries_intact()
    _check_planes(b, per, num, starts, F, fs, hop, Hs, Ws)              # the second entry reads them only
    m_, r_, p_ = b.outputs()
    assert np.array_equal(m_, exp)                                       # the uncovered pixels included: 0 over the canary
    assert np.array_equal(p_, want_prob)
    worst = worst32 = 0.0
    for f in range(F):
        cnt, x0, y0, x1, y1, bits, row, zero = (int(t) for t in r_[f])
        assert cnt == int(exp[f].sum()), (what, f, cnt, int(exp[f].sum()))
        assert (x0, y0, x1, y1) == ref.box_of(exp[f]), (what, f, (x0, y0, x1, y1), ref.box_of(exp[f]))
        first = _holders(starts, F, fs, hop, f)[0][0]
        assert row == ROW0 + V * first and zero == 0, (what, f, row, first)
        score = float(np.array([bits], np.int32).view(np.float32)[0])
        if cnt == 0:
            assert bits == 0
            continue
        r64, r32 = ref.score_refs(v[f], exp[f])
        d, d32 = abs(score - r64), abs(r32 - r64)
        worst, worst32 = max(worst, d), max(worst32, d32)
        assert d <= max(1e-6, 2.0 * d32), (what, f, score, r64, r32)
    print("%s: frame score |kernel-f64| %.3e  |fp32 torch-f64| %.3e" % (what, worst, worst32))
    # i. a null mask, a null prob, neither: the same records
    for want_mask, want_prob_ in ((False, True), (True, False), (False, False)):
        again = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
        _detect(b, F, H, W, Hs, Ws, V, fs, hop, [(0, F)], mask=want_mask, prob=want_prob_, rec=again)
        assert torch.equal(again, b.rec), (want_mask, want_prob_)
    assert np.array_equal(b.mask.cpu().numpy(), exp) and np.array_equal(b.prob.cpu().numpy().view(np.uint16), want_prob)
    b.canaries_intact()


@pytest.mark.parametrize("hop", [6, 2])
def test_the_order_and_the_split_of_the_launches_do_not_matter(hop):
    """f. The clips of case b as one launch, and as launches of 1, 3 and the rest fed in reversed order: planes, cover and every output bit-equal."""
    F, fs, Hs, Ws, views = 40, 2, 10, 12, CENTRE
    starts, x, per, num, _mean = _setup(F, fs, hop, Hs, Ws, views, seed=77 + hop)
    n = len(starts)
    outs = []
    for launches in ([list(range(n))], [list(range(4, n)), [1, 2, 3], [0]]):
        b = Buffers(F, fs, hop, Hs, Ws, Hs, Ws, 16)
        _fill_planes(b, x, starts, F, fs, hop, views, Hs, Ws, launches)
        _check_planes(b, per, num, starts, F, fs, hop, Hs, Ws)
        _detect(b, F, Hs, Ws, Hs, Ws, 1, fs, hop, [(0, F)])
        b.canaries_intact()
        outs.append((b.pbuf.clone(), b.mbuf.clone(), b.qbuf.clone(), b.rbuf.clone()))
    assert all(torch.equal(p, q) for p, q in zip(*outs)) and int(outs[0][3][8:8 + F * 8].view(F, 8)[:, 0].sum()) > 0


@pytest.mark.parametrize("Hs,Ws,H,W,views", [(10, 12, 10, 12, CENTRE), (10, 13, 10, 13, MIRRORED), (12, 16, 9, 11, TWO), (12, 16, 20, 27, TWO)])
def test_at_the_full_span_the_two_entries_are_pc_detect_frames_scaled_bit_for_bit(Hs, Ws, H, W, views):
    """g. hop = span: mask, all eight record words and probability of pc_clip_planes + pc_detect_frames_planes equal pc_detect_frames_scaled's."""
    F, fs, hop, V = 33, 2, 16, len(views)
    starts, x, per, num, _mean = _setup(F, fs, hop, Hs, Ws, views, seed=Hs * 100 + W)
    assert starts == evalstep.clip_starts(F, np.ones(F), fs)
    b = Buffers(F, fs, hop, Hs, Ws, H, W, 16)
    _fill_planes(b, x, starts, F, fs, hop, views, Hs, Ws, [list(range(len(starts)))])
    _check_planes(b, per, num, starts, F, fs, hop, Hs, Ws)
    _detect(b, F, H, W, Hs, Ws, V, fs, hop, [(0, 20), (20, 13)])
    b.canaries_intact()
    m1 = torch.full((F, H, W), PAT, dtype=torch.uint8, device="cuda")
    r1 = torch.full((F, 8), REC_CANARY, dtype=torch.int32, device="cuda")
    p1 = torch.full((F, H, W), 0, dtype=torch.int16, device="cuda")
    ops.detect_frames_scaled(torch.from_numpy(x).cuda(), views, starts, F, H, W, Hs, Ws, f_skip=fs, row0=ROW0, mask=m1, prob=p1, rec=r1)
    assert torch.equal(m1, b.mask) and torch.equal(r1, b.rec) and torch.equal(p1, b.prob)
    assert 0 < int(r1[:, 0].sum()) < F * H * W


def test_a_frame_range_inside_the_video_leaves_the_other_frames_untouched():
    """h. (f0, nf) strictly inside the video: every other frame's mask, record and probability bytes keep the canary."""
    F, fs, hop, Hs, Ws, views, f0, nf = 17, 2, 8, 10, 12, CENTRE, 5, 7
    starts, x, _per, _num, mean = _setup(F, fs, hop, Hs, Ws, views, seed=3)
    b = Buffers(F, fs, hop, Hs, Ws, Hs, Ws, 13)
    _fill_planes(b, x, starts, F, fs, hop, views, Hs, Ws, [list(range(len(starts)))])
    _detect(b, F, Hs, Ws, Hs, Ws, 1, fs, hop, [(f0, nf)])
    b.canaries_intact()
    m_, r_, p_ = b.outputs()
    rest = [f for f in range(F) if not f0 <= f < f0 + nf]
    assert (m_[rest] == PAT).all() and (r_[rest] == REC_CANARY).all() and (p_[rest] == PROB_CANARY).all()
    v, covered = ref.resample(mean, np.broadcast_to(_num, mean.shape), Hs, Ws)
    exp = ref.masks(v, covered)
    assert np.array_equal(m_[f0:f0 + nf], exp[f0:f0 + nf]) and np.array_equal(r_[f0:f0 + nf, 0], exp[f0:f0 + nf].sum(axis=(1, 2)))
    assert (r_[f0:f0 + nf, 6] == [ROW0 + _holders(starts, F, fs, hop, f)[0][0] for f in range(f0, f0 + nf)]).all() and not r_[f0:f0 + nf, 7].any()


def test_the_ops_refuse_bad_arguments():
    F, fs, hop, Hs, Ws, views = 17, 2, 8, 10, 12, CENTRE
    starts = ops.clip_hop_starts(F, fs, hop)
    assert starts == [0, 1, 8, 9] and ops.clip_planes_bytes(F, Hs, Ws, fs, hop) == 2 * F * 120 * 4 + 120
    assert ops.detect_frames_planes_ws_bytes(F, Hs, Ws) == F * 32 and ops.PLANES_MAX_FRAMES == 256
    x = torch.zeros(1, 4, 8, S, S, device="cuda")
    good = dict(logits=x, views=views, starts=starts, F=F, Hs=Hs, Ws=Ws, f_skip=fs, hop=hop)
    planes = ops.clip_planes(**good)
    assert planes.dtype == torch.uint8 and planes.numel() == ops.clip_planes_bytes(F, Hs, Ws, fs, hop)
    bad = [dict(logits=x.double()), dict(logits=x[..., :3]), dict(logits=x[:, :3]), dict(view_stride=1), dict(views=[(0, 0)]), dict(views=[]), dict(hop=3),
           dict(hop=18), dict(f_skip=0), dict(F=0), dict(planes=planes[:-1]), dict(planes=planes.view(torch.int32)), dict(planes=planes.cpu())]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.clip_planes(**dict(good, **kw))
    with pytest.raises(RuntimeError, match="pc_clip_planes"):              # what the wrapper leaves to the library: a start that is none of the rule
        ops.clip_planes(**dict(good, starts=[0, 1, 8, 10]))
    with pytest.raises(ValueError, match="clip_hop_starts"):
        ops.clip_hop_starts(17, 2, 3)
    goodf = dict(planes=planes, F=F, H=Hs, W=Ws, Hs=Hs, Ws=Ws, V=1, f_skip=fs, hop=hop)
    ops.detect_frames_planes(**goodf)
    badf = [dict(planes=planes[:-1]), dict(hop=4), dict(f0=-1), dict(f0=1, nf=F), dict(nf=0), dict(nf=257), dict(H=0),
            dict(mask=torch.zeros(F, Hs, Ws + 1, dtype=torch.uint8, device="cuda")), dict(mask=torch.zeros(F, Hs, Ws, dtype=torch.uint8)),
            dict(prob=torch.zeros(F, Hs, Ws, dtype=torch.float32, device="cuda")), dict(rec=torch.zeros(F, 7, dtype=torch.int32, device="cuda")),
            dict(ws=torch.zeros(F * 32 - 1, dtype=torch.uint8, device="cuda"))]
    for kw in badf:
        with pytest.raises(ValueError):
            ops.detect_frames_planes(**dict(goodf, **kw))
    with pytest.raises(RuntimeError, match="pc_detect_frames_planes"):
        ops.detect_frames_planes(**dict(goodf, V=33))
