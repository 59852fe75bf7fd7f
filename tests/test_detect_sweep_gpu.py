"""GPU: detect.DetectEngine.set_keep_probs / sweep at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as
tests/test_detect_score_gpu.py is sized (the tile + flip engine takes bs = 8).  The probability word 32768 cuts the engine's own masks; the
sweep at the one threshold 0.5 is score() bit for bit; the default sweep is the numpy restatement (tests/prob_hist_ref.py) of the engine's
OWN probability maps against the truth; across a second call, a second pass and packing the histograms are equal; keeping the map changes no
other field of a detection, and dropping it again is as if it had never been kept; every way to a map -- instance scores, tiled and mirrored
views, a working frame, hopped clips -- sweeps; refusals enqueue nothing; a pass plus sweep between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, step as pstep, synthetic

from tests import prob_hist_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
H0, W0 = evalstep.centre_crop(FHW[0], FHW[1], HW)
FIELDS = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first", "inst_scores", "other_score", "inst_overlaps")
WORDS = detect.threshold_words()


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


def _truth_actors(F):
    """Three actors (1, 2, 3), one value above them (7) and background, moving with the frame: any non-zero byte is truth."""
    t = np.zeros((F,) + FHW, np.uint8)
    for f in range(F):
        t[f, 8 + f:50 + f, 10:60] = 1
        t[f, 60:110, 20 + f:70 + f] = 2
        t[f, 20:90, 90:130] = 3
        t[f, 100:118, 100:136] = 7
    return t


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _probs(d):
    return d.probs.cpu().numpy().view(np.uint16)


def _differs(a, b):
    """The fields of two detections that differ, the probability map aside."""
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores", "frame_scores") if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    out += [k for k in ("masks", "imap") if (getattr(a, k) is None) != (getattr(b, k) is None) or (getattr(a, k) is not None and not torch.equal(getattr(a, k), getattr(b, k)))]
    if a.label != b.label or a.views != b.views or a.work != b.work or a.hop != b.hop:
        out.append("label/views/work/hop")
    return out


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k       # bit for bit, NaNs by position


def _same_hists(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _check_pass(de, dets, truths, labels):
    """A finished pass of any engine that kept its maps: word 32768 cuts its masks, the default sweep is the restatement of its own maps, and
    the sweep at 0.5 is score()."""
    sw = de.sweep(truths, labels)
    assert isinstance(sw, detect.SweepScore) and np.array_equal(sw.words, WORDS) and len(sw.results) == len(sw.videos[0][0, 0]) - 1 == 19
    fg = 0
    for d, t, h in zip(dets, truths, sw.videos):
        q = _probs(d)
        assert q.shape == t.shape and np.array_equal((q >= 32768).astype(np.uint8), d.masks.cpu().numpy())
        assert h.dtype == np.int32 and np.array_equal(h, ref.hist(q, t, WORDS))
        assert np.array_equal(h.reshape(h.shape[0], -1).sum(1), np.full(h.shape[0], FHW[0] * FHW[1]))
        assert np.array_equal(detect.sweep_counts(h), ref.brute_counts(q, t, WORDS))
        fg += int(h[:, :, 1:].sum())
    assert fg > 0                                                    # the synthetic weights do give probabilities at and above 0.05
    half, ps = de.sweep(truths, labels, thresholds=[0.5]), de.score(truths, labels)
    assert half.words.tolist() == [32768] and half.thresholds.tolist() == [0.5]
    _same_result(half.results[0], ps.result)
    _same_result(sw.results[9], ps.result)                           # 0.5 is the tenth of the default nineteen
    for h, v in zip(half.videos, ps.videos):
        assert np.array_equal(detect.sweep_counts(h)[0], detect.crosstab_counts(v.table)) and np.array_equal(detect.sweep_counts(h)[0], v.counts)
    return sw


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass and sweep computed once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    out = dict(eng=eng, vids=vids)
    never = eng.detect_engine(bs=BS, capacity=64)                    # an engine on which neither method is ever called
    out["never"], out["never_dets"] = never, _run(never, vids)
    de = eng.detect_engine(bs=BS, capacity=64)
    de.set_keep_probs(True)
    out["de"] = de
    out["first"] = _run(de, vids)
    out["dense"] = [(d.masks.cpu().numpy(), _probs(d)) for d in out["first"]]
    out["words"] = [r.dev.numel() for r in de.videos]
    every = [_truth_everywhere(F) for F in FRAMES]
    labels = [out["first"][0].label, (out["first"][1].label + 1) % 24, out["first"][2].label]
    out["every"], out["labels"] = every, labels
    out["sweep"] = de.sweep(every, labels)
    out["second_call"] = de.sweep(every, labels)
    out["after"] = de.results()
    _run(de, vids)
    out["second_pass"] = de.sweep(every, labels)
    _run(de, vids, pack=True)
    out["packed"] = de.sweep(every, labels)
    de.set_keep_probs(False)
    out["off_dets"] = _run(de, vids)
    out["off_probs"] = [r.prob for r in de.videos]
    de.set_keep_probs(True)
    out["on_again"] = _run(de, vids)
    return out


def test_word_32768_cuts_the_masks_and_the_sweep_is_the_restatement_and_score(world):
    sw = _check_pass(world["de"], world["on_again"], world["every"], world["labels"])
    assert _same_hists(sw.videos, world["sweep"].videos)
    assert sw.n_skipped == 0 and sw.fmAP.shape == sw.vmAP.shape == (19, 20) and sw.pixel.shape == (19, 3)
    for k in range(19):
        _same_result(sw.results[k], world["sweep"].results[k])
        assert np.array_equal(_bits(sw.fmAP[k]), _bits(sw.results[k]["fmAP"])) and np.array_equal(_bits(sw.vmAP[k]), _bits(sw.results[k]["vmAP"]))
    # pixels: tp + fn is the truth at every threshold; tp and fp fall as the threshold rises
    truth = sum(int((t != 0).sum()) for t in world["every"])
    assert (sw.pixel[:, 0] + sw.pixel[:, 2] == truth).all() and (np.diff(sw.pixel[:, 0]) <= 0).all() and (np.diff(sw.pixel[:, 1]) <= 0).all()
    for k, w in enumerate(WORDS.tolist()):
        tp = sum(int(((q >= w) & (t != 0)).sum()) for (_m, q), t in zip(world["dense"], world["every"]))
        fp = sum(int(((q >= w) & (t == 0)).sum()) for (_m, q), t in zip(world["dense"], world["every"]))
        assert sw.pixel[k].tolist() == [tp, fp, truth - tp]
    # three videos of 24 classes: the evaluator's own mean over the classes is NaN at every threshold, and best() says so
    assert np.isnan(sw.fmAP).all() and np.isnan(sw.vmAP).all()
    with pytest.raises(ValueError, match="NaN"):
        sw.best()
    with np.errstate(invalid="ignore", divide="ignore"):
        fm = [float(np.nanmean(r["frame_ious"] / r["n_tot_frames"], axis=0)[10]) for r in sw.results]
    print("f-mAP@0.5 over the classes that hold a video, per threshold: %s" % np.round(fm, 4).tolist())


def test_truth_forms_a_subset_and_a_video_without_truth(world):
    de, every, labels = world["de"], world["every"], world["labels"]
    want = world["sweep"].videos
    forms = [[t[..., None] for t in every], [torch.from_numpy(t) for t in every], [torch.from_numpy(t).cuda() for t in every]]
    for truths in forms:
        assert _same_hists(de.sweep(truths, labels).videos, want)
    sub = de.sweep([every[2], every[0], every[2]], [1, 2, 3], videos=[2, 0, 2])
    assert _same_hists(sub.videos, [want[2], want[0], want[2]])
    empty = de.sweep([], [], videos=[])
    assert empty.videos == [] and len(empty.results) == 19
    truths = [every[0], np.zeros((17,) + FHW, np.uint8), _truth_actors(40)]
    sw = de.sweep(truths, labels)
    ps = de.score(truths, labels)
    assert sw.n_skipped == ps.n_skipped == 1 and len(sw.videos) == 3 and not sw.videos[1][:, 1].any()
    _same_result(sw.results[9], ps.result)
    assert np.array_equal(sw.videos[2], ref.hist(world["dense"][2][1], truths[2], WORDS))      # truth bytes 2, 3 and 7 are truth
    assert sw.results[9]["n_vids"].sum() == 2
    sixty_four = np.linspace(0.01, 1.0, 64)
    big = de.sweep(every, labels, thresholds=sixty_four)
    for (_m, q), t, h in zip(world["dense"], every, big.videos):
        assert h.shape[2] == 65 and np.array_equal(h, ref.hist(q, t, detect.threshold_words(sixty_four)))


def test_a_second_call_a_second_pass_and_packing_give_equal_histograms(world):
    want = world["sweep"]
    for name in ("second_call", "second_pass", "packed"):
        assert _same_hists(world[name].videos, want.videos), name
        for k in range(19):
            _same_result(world[name].results[k], want.results[k])
        assert np.array_equal(world[name].pixel, want.pixel)
    assert want.videos[0] is not world["second_call"].videos[0]      # arrays of their own, not views of the staging


def test_keeping_the_map_changes_nothing_else_and_dropping_it_is_as_never(world):
    never = world["never"]
    assert world["words"] == [r.dev.numel() for r in never.videos]   # the record that leaves per video is the same
    assert never.sweep_ws is None and never.sweep_pin is None and never.tr_pin == [None, None] and never.keep_probs is False
    assert all(r.prob is None for r in never.videos) and all(p is None for p in world["off_probs"])
    for kept, after, off, again, nev, (dm, q) in zip(world["first"], world["after"], world["off_dets"], world["on_again"], world["never_dets"], world["dense"]):
        assert nev.probs is None and off.probs is None and kept.probs is not None and kept.probs.dtype == torch.int16
        assert _differs(kept, nev) == [] and _differs(off, nev) == [] and _differs(after, kept) == [] and _differs(again, kept) == []
        assert kept.inst_n is None and kept.imap is None and kept.inst_scores is None
        assert np.array_equal(_probs(after), q) and np.array_equal(after.masks.cpu().numpy(), dm)      # the sweep left the maps as they were
        assert np.array_equal(_probs(again), q)


@pytest.mark.parametrize("variant", ["instance_scores", "tile_flip", "working_frame", "clip_hop"])
def test_every_way_to_a_map_sweeps(world, variant):
    eng, vids, every, labels = world["eng"], world["vids"], world["every"], world["labels"]
    if variant == "instance_scores":                                 # the map the instance scores keep, without set_keep_probs
        de = eng.detect_engine(bs=BS, capacity=64, instances=4, min_area=3, instance_scores=True)
    elif variant == "tile_flip":
        de = eng.detect_engine(bs=8, capacity=128, tile=True, flip=True)
        de.set_keep_probs(True)
    else:
        de = eng.detect_engine(bs=BS, capacity=64)
        de.set_keep_probs(True)
        if variant == "working_frame":
            de.set_working_frame((128, 144))
        else:
            de.set_clip_hop(4)
    dets = _run(de, vids)
    sw = _check_pass(de, dets, every, labels)
    if variant == "instance_scores":
        assert de.keep_probs is False and dets[0].inst_scores is not None
        for d, (_m, q), h, base in zip(dets, world["dense"], sw.videos, world["sweep"].videos):      # the centre crop's map either way
            assert np.array_equal(_probs(d), q) and np.array_equal(h, base)
        both = eng.detect_engine(bs=BS, capacity=64, instances=4, min_area=3, instance_scores=True)
        both.set_keep_probs(True)                                    # asked for twice: one map, the same launches
        for a, b in zip(_run(both, vids), dets):
            assert _differs(a, b) == [] and torch.equal(a.probs, b.probs)
    elif variant == "tile_flip":
        assert len(dets[0].views) == 8
        border = [np.ones_like(t) for t in every]
        for t in border:
            t[:, H0:H0 + HW, W0:W0 + HW] = 0                         # everything the centre crop leaves out
        out = de.sweep(border, labels)
        centre = sum(int(((q >= int(WORDS[0])) & (t != 0)).sum()) for (_m, q), t in zip(world["dense"], border))
        assert int(out.pixel[0, 0]) > 0 and centre == 0              # what the centre crop's map cannot see
    elif variant == "working_frame":
        assert dets[0].work == (128, 144, "area")
    else:
        assert dets[2].hop == 4


def test_refusals_are_value_errors_before_anything_is_enqueued(world):
    eng, vids = world["eng"], world["vids"]
    fresh = eng.detect_engine(bs=BS, capacity=64)
    for bad in (None, 1, 0, "yes", 1.0, np.int32(1)):
        with pytest.raises(ValueError, match="set_keep_probs"):
            fresh.set_keep_probs(bad)
    assert fresh.keep_probs is False
    every, labels = world["every"], [0, 1, 2]
    with pytest.raises(ValueError, match="no finished pass"):
        fresh.sweep(every, labels)
    _run(fresh, vids)
    with pytest.raises(ValueError, match="set_keep_probs.*instance_scores"):
        fresh.sweep(every, labels)                                   # a finished pass that kept no map
    fresh.set_keep_probs(True)
    with pytest.raises(ValueError, match="set_keep_probs"):
        fresh.sweep(every, labels)                                   # the setter acts on the videos to come, not on these
    _run(fresh, vids)
    nan = float("nan")
    bad = [(dict(thresholds=[0.0]), "threshold"), (dict(thresholds=[0.5, 0.5]), "threshold"), (dict(thresholds=[0.6, 0.4]), "threshold"),
           (dict(thresholds=[1.5]), "threshold"), (dict(thresholds=[nan]), "threshold"), (dict(thresholds=[]), "threshold"),
           (dict(thresholds=np.linspace(0.01, 1.0, 65)), "threshold"), (dict(thresholds="half"), "threshold"),
           (dict(videos=[0, 1, 3]), "video"), (dict(videos=[-1, 0, 1]), "video"), (dict(videos=[0, 1]), "truths"),
           (dict(truths=every[:2]), "truths"), (dict(labels=[0, 1]), "labels"), (dict(labels=[0, 1, 24]), "label"), (dict(labels=[0, -1, 2]), "label"),
           (dict(labels=[0, 1.5, 2]), "label"), (dict(labels=[0, None, 2]), "label"),
           (dict(truths=[every[0], every[1][:16], every[2]]), "shape"), (dict(truths=[every[0], every[1], every[2][:, :, :100]]), "shape"),
           (dict(truths=[every[0], every[1][..., None, None], every[2]]), "shape"), (dict(truths=[every[0], every[1].astype(np.float32), every[2]]), "uint8"),
           (dict(truths=[every[0], every[1].astype(np.int32), every[2]]), "uint8"), (dict(truths=[every[0], every[1].tolist(), every[2]]), "uint8")]
    for kw, word in bad:
        args = dict(truths=every, labels=labels)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fresh.sweep(**args)
    assert fresh.sweep_ws is None and fresh.sweep_pin is None and fresh.tr_pin == [None, None] and fresh.tr_done == [None, None]      # nothing went up
    assert _same_hists(fresh.sweep(every, world["labels"]).videos, world["sweep"].videos)
    fresh.begin()
    with pytest.raises(ValueError, match="no finished pass"):
        fresh.sweep(every, labels)
    records = eng.detect_engine(bs=BS, capacity=64, masks=False)     # the map needs no mask
    records.set_keep_probs(True)
    _run(records, vids[:1])
    assert np.array_equal(records.sweep(every[:1], [0]).videos[0], world["sweep"].videos[0])


def test_a_pass_and_sweep_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with its map kept and a sweep on the step engine's weights, train step, against the same two steps on a
    fresh engine: the second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are
    equal bit for bit."""
    eng, de = world["eng"], world["de"]
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    truths = [_truth_actors(F) for F in FRAMES[:2]]
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            dets = _run(de, world["vids"][:2])
            sw = de.sweep(truths, [0, 1])
            for d, t, h in zip(dets, truths, sw.videos):
                assert np.array_equal(h, ref.hist(_probs(d), t, WORDS))
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
