"""GPU: detect.DetectEngine(instance_links=L) at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as
tests/test_instances_gpu.py is sized (the tile + flip engine takes bs = 8).  Per video the overlap record is exact against the restatement of
tests/instance_links_ref.py applied to the engine's OWN map of ranks; across the ways of batching the records are equal; together with
instance_scores both records decode to what each gives alone; instance_tubes(link="mask") is the host function on the decoded fields; an
engine without the option is today's engine in every field and buffer size; a pass between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, ops, step as pstep, synthetic

from tests import instance_links_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
K, MIN_AREA, L = 8, 3, 2


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


def _differs(a, b, links, maps=True):
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores", "frame_scores") if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    out += [k for k in (("masks", "imap") if maps else ("masks",)) if not torch.equal(getattr(a, k), getattr(b, k))]
    if a.label != b.label or a.views != b.views:
        out.append("label/views")
    if links and not np.array_equal(a.inst_overlaps, b.inst_overlaps):
        out.append("inst_overlaps")
    return out


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass computed once and shared.  Only the last test of the file trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    kw = dict(instances=K, min_area=MIN_AREA, instance_maps=True)
    de = eng.detect_engine(bs=BS, capacity=64, instance_links=L, **kw)
    out = dict(eng=eng, vids=vids, de=de, first=_run(de, vids), again=_run(de, vids), packed=_run(de, vids, pack=True))
    out["tile_flip"] = _run(eng.detect_engine(bs=8, capacity=128, tile=True, flip=True, instance_links=L, **kw), vids)
    out["nomaps"] = _run(eng.detect_engine(bs=BS, capacity=64, instances=K, min_area=MIN_AREA, instance_links=L), vids)
    out["scored"] = _run(eng.detect_engine(bs=BS, capacity=64, instance_scores=True, instance_links=L, **kw), vids)
    out["scores_only"] = _run(eng.detect_engine(bs=BS, capacity=64, instance_scores=True, **kw), vids)
    out["today"] = _run(eng.detect_engine(bs=BS, capacity=64, **kw), vids)
    return out


def _against_restatement(dets, what):
    """The overlaps of `dets` against the restatement on their own imap -> (frames, labelled frames, overflow frames, pairs of frames that
    share foreground, those of them with an overflow frame on either side)."""
    seen = some = over = shared = through_k = 0
    for F, d in zip(FRAMES, dets):
        imap = d.imap.cpu().numpy()
        assert imap.shape == (F,) + FHW and ((imap != 0) == (d.masks.cpu().numpy() != 0)).all()
        want = ref.overlaps(imap, K, L)
        assert d.inst_overlaps.dtype == np.int32 and d.inst_overlaps.shape == (F, L, K + 1, K + 1)
        assert np.array_equal(d.inst_overlaps, want), (what, F, np.argwhere(d.inst_overlaps != want)[:8].tolist())
        ok = (d.inst_flags & 1) == 0
        pix = ref.slot_pixels(imap, K)
        for f in range(F):
            assert int(pix[f].sum()) == int(d.counts[f]), (what, F, f)
            if ok[f]:
                kept = int(d.inst_kept[f])
                assert np.array_equal(pix[f, :kept], d.inst_areas[f, :kept]) and not pix[f, kept:K].any()
            else:                                                     # over the run cap: the map is 255 on all foreground, one substituted instance
                assert not pix[f, :K].any() and pix[f, K] == d.counts[f] == d.inst_areas[f, 0] and d.inst_kept[f] == 1
            for lag in range(L):
                g = f + lag + 1
                rec = d.inst_overlaps[f, lag]
                if g >= F:
                    assert not rec.any()
                    continue
                assert (rec.sum(1) <= pix[f]).all() and (rec.sum(0) <= pix[g]).all()
                if not ok[f]:
                    assert not rec[:K].any()
                if not ok[g]:
                    assert not rec[:, :K].any()
                if rec.any():
                    shared += 1
                    through_k += int(not (ok[f] and ok[g]))
        seen += F; some += int((ok & (d.inst_kept > 0)).sum()); over += int((~ok).sum())
    print("%s: %d frames, %d labelled with an instance, %d over the run cap; %d pairs of frames share foreground, %d of them with a frame over the cap"
          % (what, seen, some, over, shared, through_k))
    return seen, some, over, shared, through_k


def test_overlaps_are_exact_on_the_engines_own_maps(world):
    seen, some, over, shared, through_k = _against_restatement(world["first"], "centre")
    # both paths: labelled frames, and overflow frames that link through slot K
    assert seen == sum(FRAMES) and some > 0 and over > 0 and shared > 0 and through_k > 0


def test_mask_linking_is_the_host_function_on_the_decoded_fields(world):
    for d in world["first"]:
        for kw in (dict(), dict(max_gap=1), dict(iou_min=0.1, max_gap=1, min_len=2)):
            got = d.instance_tubes(link="mask", **kw)
            want = detect.link_instance_tubes_by_mask(d.inst_kept, d.inst_boxes, d.inst_areas, d.frame_scores, d.inst_overlaps, d.inst_flags, **kw)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and a[4] == b[4]
        with pytest.raises(ValueError, match="max_gap"):
            d.instance_tubes(link="mask", max_gap=L)
        # the default is today's linking
        box = d.instance_tubes()
        want = detect.link_instance_tubes(d.inst_kept, d.inst_boxes, d.inst_areas, d.frame_scores)
        assert [(t[0], t[1], t[3].tolist(), t[4]) for t in box] == [(t[0], t[1], t[3].tolist(), t[4]) for t in want]
    # a frame over the cap holds the frame's whole foreground: two such frames in a row with any common pixel link at their mask IoU
    d = world["first"][2]
    over = (d.inst_flags & 1) != 0
    tubes = d.instance_tubes(link="mask", iou_min=0.0)
    for f in range(len(over) - 1):
        if over[f] and over[f + 1] and d.inst_kept[f] and d.inst_kept[f + 1]:
            assert any(t0 <= f and f + 1 <= t1 and areas[f - t0] == d.counts[f] and areas[f + 1 - t0] == d.counts[f + 1] for t0, t1, _b, areas, _s in tubes), f


def test_batching_a_second_pass_and_the_views(world):
    first = world["first"]
    for name in ("again", "packed"):
        assert [_differs(a, b, True) for a, b in zip(first, world[name])] == [[]] * len(first), name
    tf = world["tile_flip"]
    assert all(len(d.views) == 8 for d in tf)
    seen, _some, _over, shared, _k = _against_restatement(tf, "tile + flip")
    assert seen == sum(FRAMES) and shared > 0
    for a, b in zip(first, world["nomaps"]):                          # the map of ranks is made for the overlaps, and kept to the engine
        assert b.imap is None and a.imap is not None
        assert _differs(a, b, True, maps=False) == []


def test_together_with_instance_scores_both_records_decode(world):
    """The overlap words lie behind the score words: the score decoder must stop where they begin."""
    for a, s, o in zip(world["scored"], world["scores_only"], world["first"]):
        assert _differs(a, s, False) == [] and _differs(a, o, True) == []
        assert np.array_equal(a.inst_scores, s.inst_scores) and np.array_equal(a.other_score, s.other_score) and torch.equal(a.probs, s.probs)
        assert a.inst_scores.shape == (len(a.counts), K) and s.inst_overlaps is None
        got = a.instance_tubes(link="mask", max_gap=1)
        want = detect.link_instance_tubes_by_mask(a.inst_kept, a.inst_boxes, a.inst_areas, a.frame_scores, a.inst_overlaps, a.inst_flags, max_gap=1,
                                                  inst_scores=a.inst_scores)
        assert [(t[0], t[1], t[4]) for t in got] == [(t[0], t[1], t[4]) for t in want]


def test_the_option_off_is_todays_engine(world):
    eng, first = world["eng"], world["first"]
    for a, b in zip(first, world["today"]):
        assert _differs(a, b, False) == []                           # nor do the overlaps change an existing field
        assert b.inst_overlaps is None and a.inst_scores is a.other_score is a.probs is None
        with pytest.raises(ValueError, match="overlaps"):
            b.instance_tubes(link="mask")
    kw = dict(bs=BS, capacity=64, instances=K, min_area=MIN_AREA)
    engines = [eng.detect_engine(**kw), eng.detect_engine(instance_links=0, **kw), eng.detect_engine(instance_scores=True, **kw),
               eng.detect_engine(instance_links=L, **kw), eng.detect_engine(instance_scores=True, instance_links=L, **kw)]
    for de in engines:
        de.begin()
        de.add_video(world["vids"][1])
    F, C = FRAMES[1], engines[0].C
    base, score, link = F * 8 + C + 2 + F * (4 + 6 * K), F * 3 * (K + 1), F * L * (K + 1) ** 2
    for de in engines[:2]:
        r = de.videos[0]
        assert r.dev.numel() == base and r.imap is None and r.prob is None and r.link_words == 0
    assert engines[2].videos[0].dev.numel() == base + score
    r = engines[3].videos[0]
    assert r.dev.numel() == base + link and r.imap.shape == (F,) + FHW and r.prob is None          # behind the instance records: nothing before moves
    r = engines[4].videos[0]
    assert r.dev.numel() == base + score + link and r.score_words == score and r.link_words == link
    dets = [de.results()[0] for de in engines]
    assert np.array_equal(dets[3].inst_overlaps, first[1].inst_overlaps) and np.array_equal(dets[4].inst_overlaps, first[1].inst_overlaps)
    assert np.array_equal(dets[4].inst_scores, dets[2].inst_scores) and dets[3].imap is None
    with pytest.raises(ValueError, match="instances"):
        eng.detect_engine(bs=BS, capacity=64, instance_links=L)


def test_a_linking_pass_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with instance links on the step engine's weights, train step, against the same two steps on a fresh engine:
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
            assert all(d.inst_overlaps is not None for d in dets)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
