"""GPU: detect.DetectEngine.set_mask_threshold / recut at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as
tests/test_detect_sweep_gpu.py is sized (the tile + flip engine takes bs = 8).  The sweep and the cut agree: recut(sw.thresholds[k]) then
score() is sw.results[k] bit for bit, at thresholds taken from the pass's own probability words so that the cuts differ; recut(0.5) of a
plain pass gives its masks, records and instances again (frame scores within 1e-5); a pass under set_mask_threshold(t) is a kept pass plus
recut(t) in every field, on every route to a map; recut works in place, on the picked videos alone, and can be undone by a second recut;
refusals enqueue nothing; a pass plus a recut between two train steps changes nothing."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, step as pstep, synthetic

from tests import prob_cut_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
H0, W0 = evalstep.centre_crop(FHW[0], FHW[1], HW)
FIELDS = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first", "inst_scores", "other_score", "inst_overlaps")
DENSE = ("masks", "imap", "probs")
INST = dict(instances=4, min_area=3, instance_scores=True, instance_links=2, instance_maps=True)
BAD_THRESHOLDS = (0.0, -0.1, 1.5, float("nan"), float("inf"), "half", None, [0.5], [0.2, 0.4], True, False)


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


def _truth_everywhere(F):
    """In {0, 1}, inside the centre crop, in every frame (tests/test_detect_score_gpu.py)."""
    t = np.zeros((F,) + FHW, np.uint8)
    t[:, 30:70, 40:90] = 1
    t[::2, 10:110, 20:40] = 1
    return t


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _snap(d):
    """A detection with its device tensors copied to the host: recut works in place, so what a pass gave has to be kept to be compared."""
    s = SimpleNamespace(**{k: getattr(d, k) for k in FIELDS + ("class_score", "class_scores", "frame_scores", "label", "views", "work", "hop", "threshold")})
    for k in DENSE:
        t = getattr(d, k)
        setattr(s, k, None if t is None else t.cpu().numpy().copy())
    return s


def _snaps(dets):
    return [_snap(d) for d in dets]


def _dense(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _differs(a, b, scores=True, probs=True):
    """The fields of two detections (or their snapshots) that differ; scores=False: the frame scores aside, probs=False: the map aside."""
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores") + (("frame_scores",) if scores else ()) if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    for k in DENSE if probs else DENSE[:2]:
        x, y = _dense(getattr(a, k)), _dense(getattr(b, k))
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            out.append(k)
    if a.label != b.label or a.views != b.views or a.work != b.work or a.hop != b.hop:
        out.append("label/views/work/hop")
    return out


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k       # bit for bit, NaNs by position


def _words(q):
    return q.view(np.uint16)


def _check_cut(d, word, masks=True):
    """A detection cut at `word`: its mask is its own map >= word and its records are the restatement's, bit for bit."""
    q = _words(_dense(d.probs))
    wm, wr = ref.cut(q, word)
    if masks:
        assert np.array_equal(_dense(d.masks), wm)
    assert np.array_equal(d.counts, wr[:, 0]) and np.array_equal(d.boxes, wr[:, 1:5])
    assert np.array_equal(np.asarray(d.frame_scores, np.float32).view(np.int32), wr[:, 5])
    assert d.threshold[1] == word and detect.cut_word(d.threshold[0]) == word
    return int(wr[:, 0].sum())


def _engine(eng, variant):
    """-> (engine, videos' pack flag).  The routes to a mask."""
    if variant == "instances":
        return eng.detect_engine(bs=BS, capacity=64, **INST), False
    if variant == "tile_flip":
        return eng.detect_engine(bs=8, capacity=128, tile=True, flip=True), False
    if variant == "no_masks":
        return eng.detect_engine(bs=BS, capacity=64, masks=False), False
    de = eng.detect_engine(bs=BS, capacity=64)
    if variant == "working_frame":
        de.set_working_frame((128, 144))
    elif variant == "clip_hop":
        de.set_clip_hop(4)
    return de, variant == "pack"


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2), the centre-crop engine with its map kept, its pass and the thresholds taken from that pass's own words, computed
    once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    out = dict(eng=eng, vids=vids)
    never = eng.detect_engine(bs=BS, capacity=64)                    # an engine on which no method of the feature is ever called
    out["never"] = never
    out["never_dets"] = _snaps(_run(never, vids))
    de = eng.detect_engine(bs=BS, capacity=64)
    de.set_keep_probs(True)
    out["de"] = de
    out["handed"] = _run(de, vids)                                   # the objects a user holds: their tensors are the engine's
    out["plain"] = _snaps(out["handed"])
    every = [_truth_everywhere(F) for F in FRAMES]
    out["every"], out["labels"] = every, [out["plain"][0].label, (out["plain"][1].label + 1) % 24, out["plain"][2].label]
    # Thresholds from the pass's own maps: the synthetic weights' probabilities hover around 0.5, so fixed thresholds could all cut the same
    # pixels.  The words at five quantiles of the covered (non-zero) probability words, and the word of a half, each handed back as
    # w / 65535 -- the round trip cut_word guarantees.
    q = np.concatenate([_words(s.probs).reshape(-1) for s in out["plain"]])
    w = np.unique(np.concatenate([np.quantile(q[q > 0], [0.1, 0.3, 0.5, 0.7, 0.9]).astype(np.int64), [32768]]))
    out["words"] = np.clip(w, 1, 65535)
    out["thresholds"] = out["words"] / 65535.0
    out["t"] = float([t for t, x in zip(out["thresholds"], out["words"]) if x != 32768][1])  # the threshold of the other tests: not a half
    return out


def test_the_sweep_and_the_cut_agree(world):
    de, every, labels = world["de"], world["every"], world["labels"]
    sw = de.sweep(every, labels, thresholds=world["thresholds"])
    assert np.array_equal(sw.words, world["words"]) and len(sw.results) >= 3
    totals = {}
    for k in range(len(sw.results)):
        word, t = int(sw.words[k]), float(sw.thresholds[k])
        dets = de.recut(t)
        assert len(dets) == 3
        ps = de.score(every, labels)
        _same_result(ps.result, sw.results[k])
        totals[k] = 0
        for d, plain, h, v in zip(dets, world["plain"], sw.videos, ps.videos):
            assert d.threshold == (t, word)
            assert np.array_equal(v.counts, detect.sweep_counts(h)[k])
            assert np.array_equal(_words(_dense(d.probs)), _words(plain.probs))              # the map is read, never written
            totals[k] += _check_cut(d, word)
            assert int(d.masks.sum()) == int(d.counts.sum())
            assert d.label == plain.label and np.array_equal(_bits(d.class_scores), _bits(plain.class_scores)) and d.views == plain.views
    print("positive pixels per threshold word: %s" % {int(sw.words[k]): n for k, n in totals.items()})
    assert len(set(totals.values())) >= 3                            # three cuts that differ, or the test shows nothing
    assert sorted(totals.values(), reverse=True) == list(totals.values())                    # a higher word never adds a pixel
    # the sweep after the cuts is the sweep before them: the maps are as they were
    again = de.sweep(every, labels, thresholds=world["thresholds"])
    for k in range(len(sw.results)):
        _same_result(again.results[k], sw.results[k])
    de.recut(0.5)                                                    # (leave the pass as the other tests expect it: at a half)


def test_recut_at_a_half_of_a_plain_pass_gives_the_pass_again(world):
    eng, vids = world["eng"], world["vids"]
    inst, _ = _engine(eng, "instances")
    for de, own in ((world["de"], None), (inst, True)):
        plain = world["plain"] if own is None else _snaps(_run(de, vids))
        for d, p in zip(de.recut(0.5), plain):
            assert p.threshold is None and d.threshold == (0.5, 32768)
            assert _differs(d, p, scores=False) == []                # masks, counts, boxes, instances, maps of ranks, scores, overlaps, class
            assert np.abs(np.asarray(d.frame_scores, np.float64) - np.asarray(p.frame_scores, np.float64)).max() <= 1e-5
            _check_cut(d, 32768)
            if own:
                assert d.inst_n is not None and d.imap is not None and d.inst_scores is not None and d.inst_overlaps is not None
    assert int(sum(p.inst_n.sum() for p in plain)) > 0               # (the instance engine did find components to compare)


def test_a_pass_under_a_threshold_is_a_kept_pass_cut_again(world):
    eng, vids, t = world["eng"], world["vids"], world["t"]
    word = detect.cut_word(t)
    assert word != 32768
    de = eng.detect_engine(bs=BS, capacity=64)
    de.set_mask_threshold(t)
    assert de.mask_threshold == (t, word) and de.keep_probs is False
    under = _snaps(_run(de, vids))
    again = _snaps(world["de"].recut(t))
    world["de"].recut(0.5)
    for a, b, p in zip(under, again, world["plain"]):
        assert a.threshold == b.threshold == (t, word)
        assert _differs(a, b) == []                                  # every field, frame scores and map included
        assert np.array_equal(a.probs, p.probs) and set(_differs(a, p, scores=False)) <= {"counts", "boxes", "masks"}      # the cut and nothing else
        _check_cut(a, word)
    assert sum(int(a.counts.sum()) for a in under) != sum(int(p.counts.sum()) for p in world["plain"])
    # back to None: as if no threshold had ever been set
    de.set_mask_threshold(None)
    assert de.mask_threshold is None
    off = _run(de, vids)
    assert all(r.prob is None and r.cut is None for r in de.videos)
    for a, nev in zip(off, world["never_dets"]):
        assert a.threshold is None and a.probs is None and _differs(a, nev) == []
    assert world["never"].ws_cut is None and world["never"].mask_threshold is None


@pytest.mark.parametrize("variant", ["instances", "tile_flip", "working_frame", "clip_hop", "pack", "no_masks"])
def test_the_routes(world, variant):
    eng, vids, t = world["eng"], world["vids"], world["t"]
    word = detect.cut_word(t)
    de, pack = _engine(eng, variant)
    de.set_mask_threshold(t)
    under = _snaps(_run(de, vids, pack))
    kept, _ = _engine(eng, variant)
    kept.set_keep_probs(True)
    first = _snaps(_run(kept, vids, pack))
    again = _snaps(kept.recut(t))
    for a, b, f in zip(under, again, first):
        assert a.threshold == b.threshold == (t, word) and f.threshold is None
        assert _differs(a, b) == []
        assert np.array_equal(a.probs, f.probs)
        if f.masks is not None:
            assert np.array_equal(f.masks, (_words(f.probs) >= 32768).astype(np.uint8))      # (the kept pass itself was cut by seg_positive)
        _check_cut(a, word, masks=variant != "no_masks")
    if variant == "instances":
        assert under[2].inst_n is not None and under[2].imap is not None and under[2].inst_scores is not None and under[2].inst_overlaps.shape[1] == 2
        assert sum(int(a.inst_n.sum()) for a in under) > 0
    elif variant == "tile_flip":
        assert len(under[0].views) == 8
    elif variant == "working_frame":
        assert under[0].work == (128, 144, "area")
    elif variant == "clip_hop":
        assert under[2].hop == 4
    elif variant == "no_masks":
        assert all(a.masks is None for a in under + again)
        with_masks = _snaps(world["de"].recut(t))
        world["de"].recut(0.5)
        for a, m in zip(under, with_masks):                          # records only, equal to the records of the engine with masks
            assert _differs(a, m) == ["masks"]
    else:
        for a, m in zip(under, _snaps(world["de"].recut(t))):        # packing moves no pixel
            assert _differs(a, m) == []
        world["de"].recut(0.5)


def test_recut_works_in_place_on_the_picked_videos_and_can_be_undone(world):
    de, t = world["de"], world["t"]
    handed, plain = world["handed"], world["plain"]
    half = _snaps(de.recut(0.5))
    dev_before = [r.dev.clone() for r in de.videos]
    pins = [r.pin for r in de.videos]
    one = de.recut(t, videos=[1])
    assert len(one) == 1 and one[0].threshold == (t, detect.cut_word(t))
    assert one[0].masks is handed[1].masks and one[0].probs is handed[1].probs                 # the same tensors: the new contents show through
    assert np.array_equal(handed[1].counts, plain[1].counts)                                   # ... the host arrays handed out earlier do not change
    assert not np.array_equal(one[0].counts, plain[1].counts)
    for v in (0, 2):                                                 # not picked: masks, maps and records bit-identical
        assert torch.equal(de.videos[v].dev, dev_before[v]) and de.videos[v].pin is pins[v]
        assert np.array_equal(_dense(handed[v].masks), half[v].masks) and np.array_equal(_dense(handed[v].probs), half[v].probs)
        assert de.videos[v].cut == (0.5, 32768)
    assert de.videos[1].pin is not pins[1]
    # mask_runs, called afterwards, sees the re-cut pass
    runs = de.mask_runs()
    for r, d in zip(runs, handed):
        want = detect.MaskRuns.from_dense(_dense(d.masks))
        assert r.shape == want.shape and np.array_equal(r.offsets, want.offsets) and np.array_equal(r.runs, want.runs)
    assert np.array_equal(runs[1].dense(), (_words(plain[1].probs) >= detect.cut_word(t)).astype(np.uint8))
    assert np.array_equal(runs[0].dense(), plain[0].masks)
    # a second recut at the first threshold restores the first result, in every order of the videos
    back = _snaps(de.recut(0.5, videos=[2, 1, 0]))[::-1]
    for a, b in zip(back, half):
        assert _differs(a, b) == [] and a.threshold == b.threshold == (0.5, 32768)
    assert de.recut(0.5, videos=[]) == []
    # a second pass after a recut is unaffected
    de.recut(t)
    for a, p in zip(_run(de, world["vids"]), plain):
        assert a.threshold is None and _differs(a, p) == []
    world["handed"] = de.results()


def test_refusals_are_value_errors_with_nothing_allocated_or_enqueued(world):
    eng, vids = world["eng"], world["vids"]
    fresh = eng.detect_engine(bs=BS, capacity=64)
    for bad in BAD_THRESHOLDS:
        if bad is None:
            continue
        with pytest.raises(ValueError, match="set_mask_threshold"):
            fresh.set_mask_threshold(bad)
    assert fresh.mask_threshold is None
    with pytest.raises(ValueError, match="no finished pass"):
        fresh.recut(0.5)
    dets = _run(fresh, vids)
    with pytest.raises(ValueError, match="set_keep_probs.*instance_scores|instance_scores.*set_keep_probs") as e:
        fresh.recut(0.5)                                             # a finished pass that kept no map
    assert "set_mask_threshold" in str(e.value)
    fresh.set_mask_threshold(0.4)
    with pytest.raises(ValueError, match="set_mask_threshold"):
        fresh.recut(0.5)                                             # the setter acts on the videos to come, not on these
    fresh.set_mask_threshold(None)
    fresh.set_keep_probs(True)
    dets = _snaps(_run(fresh, vids))
    state = [(r.pin, r.cut, r.dev.clone()) for r in fresh.videos]
    stage = (fresh.pin_i, fresh.pin_off, len(fresh.pins))
    for bad in BAD_THRESHOLDS:
        with pytest.raises(ValueError, match="recut"):
            fresh.recut(bad)
    for bad in ([3], [-1], [0, 1, 3], [0, 7]):
        with pytest.raises(ValueError, match="video"):
            fresh.recut(0.4, videos=bad)
    mixed = eng.detect_engine(bs=BS, capacity=64)                    # one video keeps a map, the other does not: refused as a whole
    mixed.begin()
    mixed.set_keep_probs(True)
    mixed.add_video(vids[0])
    mixed.set_keep_probs(False)
    mixed.add_video(vids[1])
    mixed.results()
    with pytest.raises(ValueError, match="video 1 keeps no probability map"):
        mixed.recut(0.4)
    assert mixed.ws_cut is None and mixed.videos[0].cut is None
    assert len(mixed.recut(0.4, videos=[0])) == 1                    # ... the one that keeps it can be cut
    assert fresh.ws_cut is None and (fresh.pin_i, fresh.pin_off, len(fresh.pins)) == stage
    for r, (pin, cut, dev) in zip(fresh.videos, state):
        assert r.pin is pin and r.cut is cut and torch.equal(r.dev, dev)
    for a, p in zip(fresh.recut(0.5), dets):
        assert _differs(a, p, scores=False) == []
    fresh.begin()
    with pytest.raises(ValueError, match="no finished pass"):
        fresh.recut(0.5)


def test_a_pass_and_a_recut_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with its map kept and a recut on the step engine's weights, train step, against the same two steps on a
    fresh engine: the second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are
    equal bit for bit."""
    eng, de = world["eng"], world["de"]
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            _run(de, world["vids"][:2])
            for d in de.recut(world["t"]):
                _check_cut(d, detect.cut_word(world["t"]))
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
