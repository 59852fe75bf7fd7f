"""GPU: detect.DetectEngine(instance_scores=True) at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as
tests/test_instances_gpu.py is sized (the tile + flip engine takes bs = 8).  Per frame the score record is exact against the restatement of
tests/instance_scores_ref.py applied to the engine's OWN probability map and map of ranks, its pixel counts are the instance areas and the
frame's count, and the mean over all foreground is the frame score the detect kernel left; across the ways of batching the scores are equal;
an engine without the option is today's engine in every field and buffer size; a pass between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, ops, step as pstep, synthetic

from tests import instance_scores_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
K, MIN_AREA = 8, 3


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


FIELDS = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")


def _differs(a, b, scores):
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores", "frame_scores") if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    out += [k for k in ("masks", "imap") if not ((getattr(a, k) is None and getattr(b, k) is None) or torch.equal(getattr(a, k), getattr(b, k)))]
    if a.label != b.label or a.views != b.views:
        out.append("label/views")
    if scores:
        out += [k for k in ("inst_scores", "other_score") if not np.array_equal(getattr(a, k), getattr(b, k))]
        if not torch.equal(a.probs, b.probs):
            out.append("probs")
    return out


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass computed once and shared.  Only the last test of the file trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    kw = dict(instances=K, min_area=MIN_AREA, instance_maps=True)
    de = eng.detect_engine(bs=BS, capacity=64, instance_scores=True, **kw)
    out = dict(eng=eng, vids=vids, de=de, first=_run(de, vids), again=_run(de, vids), packed=_run(de, vids, pack=True))
    out["tile_flip"] = _run(eng.detect_engine(bs=8, capacity=128, tile=True, flip=True, instance_scores=True, **kw), vids)
    out["nomaps"] = _run(eng.detect_engine(bs=BS, capacity=64, instances=K, min_area=MIN_AREA, instance_scores=True), vids)
    out["off"] = _run(eng.detect_engine(bs=BS, capacity=64, instance_scores=False, **kw), vids)
    out["today"] = _run(eng.detect_engine(bs=BS, capacity=64, **kw), vids)
    return out


def _against_restatement(dets, what):
    """Every score field of `dets` against the restatement on their own probs and imap -> (frames, labelled frames, overflow frames)."""
    seen = some = over = 0
    worst = 0.0
    for F, d in zip(FRAMES, dets):
        probs, imap = d.probs.cpu().numpy().view(np.uint16), d.imap.cpu().numpy()
        assert d.probs.dtype == torch.int16 and probs.shape == imap.shape == (F,) + FHW
        assert ((imap != 0) == (d.masks.cpu().numpy() != 0)).all()
        assert (probs[imap != 0] >= 32768).all()                      # a positive pixel has sigmoid >= 0.5
        sums, npix = ref.slot_sums(imap, probs, K)
        want_sc, want_other = detect.score_instances(sums, npix, d.inst_kept, d.inst_flags)
        assert d.inst_scores.dtype == np.float64 and d.inst_scores.shape == (F, K) and d.other_score.shape == (F,)
        assert np.array_equal(d.inst_scores, want_sc) and np.array_equal(d.other_score, want_other), (what, F)      # the sums are exact
        ok = (d.inst_flags & 1) == 0
        for f in range(F):
            assert int(npix[f].sum()) == int(d.counts[f]), (what, F, f)
            if ok[f]:
                kept = int(d.inst_kept[f])
                assert np.array_equal(npix[f, :kept], d.inst_areas[f, :kept]) and not npix[f, kept:K].any(), (what, F, f)
                assert np.array_equal(d.inst_scores[f, :kept], sums[f, :kept] / (65535.0 * npix[f, :kept])) and not d.inst_scores[f, kept:].any()
            else:                                                     # over the run cap: the map is 255 on all foreground, one substituted instance
                assert not npix[f, :K].any() and npix[f, K] == d.counts[f] == d.inst_areas[f, 0] and d.inst_kept[f] == 1
                assert d.inst_scores[f, 0] == d.other_score[f] == sums[f, K] / (65535.0 * npix[f, K]) and not d.inst_scores[f, 1:].any()
            if d.counts[f]:
                mean = float(sums[f].sum()) / (65535.0 * float(d.counts[f]))
                dist = abs(mean - float(d.frame_scores[f]))
                worst = max(worst, dist)
                # each q lies within 0.5 + 2^-8 of 65535 p, i.e. 7.7e-6 of p, plus the float32 frame score's rounding (3e-8 below 1)
                assert dist <= 1e-5, (what, F, f, mean, float(d.frame_scores[f]))
                assert (0.5 <= d.inst_scores[f, :int(d.inst_kept[f])]).all() and (d.inst_scores[f] <= 1.0).all()
            else:
                assert not sums[f].any() and d.other_score[f] == 0.0 and not d.inst_scores[f].any()
        seen += F; some += int((ok & (d.inst_kept > 0)).sum()); over += int((~ok).sum())
    print("%s: %d frames, %d labelled, %d over the run cap; max |mean of q - frame score| = %.3e" % (what, seen, some, over, worst))
    return seen, some, over


def test_scores_are_exact_on_the_engines_own_maps_and_meet_the_frame_score(world):
    seen, some, over = _against_restatement(world["first"], "centre")
    assert seen == sum(FRAMES) and some > 0 and over > 0              # both paths: labelled frames and the substitute of the overflow frames
    for d in world["first"]:
        tubes = d.instance_tubes()
        plain = detect.link_instance_tubes(d.inst_kept, d.inst_boxes, d.inst_areas, d.frame_scores)
        assert [(t[0], t[1]) for t in tubes] == [(t[0], t[1]) for t in plain]
        for t0, t1, _b, areas, score in tubes:
            det = [t for t in range(t0, t1 + 1) if areas[t - t0]]
            assert 0.5 <= score <= 1.0 and det
    # two instances of one frame carry their own numbers
    assert any(len(set(d.inst_scores[f, :int(d.inst_kept[f])].tolist())) > 1 for d in world["first"] for f in range(len(d.counts)) if d.inst_kept[f] > 1)


def test_batching_a_second_pass_and_the_views(world):
    first = world["first"]
    for name in ("again", "packed"):
        assert [_differs(a, b, True) for a, b in zip(first, world[name])] == [[]] * len(first), name
    tf = world["tile_flip"]
    assert all(len(d.views) == 8 for d in tf)
    seen, _some, _over = _against_restatement(tf, "tile + flip")
    assert seen == sum(FRAMES)
    for a, b in zip(first, world["nomaps"]):                          # the map of ranks is made for the scores, and kept to the engine
        assert b.imap is None and a.imap is not None
        assert np.array_equal(a.inst_scores, b.inst_scores) and np.array_equal(a.other_score, b.other_score) and torch.equal(a.probs, b.probs)


def test_the_option_off_is_todays_engine(world):
    eng, first = world["eng"], world["first"]
    for name in ("off", "today"):
        for a, b in zip(first, world[name]):
            assert _differs(a, b, False) == [], name                 # nor do the scores change an existing field
            assert b.inst_scores is b.other_score is b.probs is None
    for d in world["today"]:
        t = d.instance_tubes()
        want = detect.link_instance_tubes(d.inst_kept, d.inst_boxes, d.inst_areas, d.frame_scores)
        assert [x[4] for x in t] == [x[4] for x in want]
    engines = [eng.detect_engine(bs=BS, capacity=64, instances=K, min_area=MIN_AREA), eng.detect_engine(bs=BS, capacity=64, instances=K, min_area=MIN_AREA, instance_scores=False),
               world["de"]]
    for de in engines:
        de.begin()
        de.add_video(world["vids"][1])
    F, C = FRAMES[1], engines[0].C
    base = F * 8 + C + 2 + F * (4 + 6 * K)
    for de in engines[:2]:
        r = de.videos[0]
        assert r.dev.numel() == base and r.imap is None and r.prob is None
    r = engines[2].videos[0]
    assert r.dev.numel() == base + F * 3 * (K + 1) and r.prob.shape == r.imap.shape == (F,) + FHW      # behind the instance records: nothing before moves
    for de in engines:
        de.results()
    with pytest.raises(ValueError, match="instances"):
        eng.detect_engine(bs=BS, capacity=64, instance_scores=True)


def test_a_scoring_pass_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with instance scores on the step engine's weights, train step, against the same two steps on a fresh engine:
    the second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are equal bit for
    bit."""
    eng, de = world["eng"], world["de"]
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            dets = _run(de, world["vids"][:2])
            assert all(d.inst_scores is not None and d.probs is not None for d in dets)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
