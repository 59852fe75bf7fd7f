"""GPU: detect.DetectEngine.score at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as tests/test_mask_runs_gpu.py is sized
(the tile + flip engine takes bs = 8).  The tables of a pass are the numpy restatement (tests/map_crosstab_ref.py) of the engine's OWN masks
and maps of ranks against the truth; on a centre-crop engine with a truth that is zero outside the crop they give the very tables
evalstep.EvalEngine leaves; a tiled and mirrored pass sees the truth the crop leaves out; across a second call, a second pass and packing the
tables are equal; the call changes no field of a detection and no buffer size; a pass plus score between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, step as pstep, synthetic

from tests import map_crosstab_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
K, MIN_AREA, ACTORS = 8, 3, 3
H0, W0 = evalstep.centre_crop(FHW[0], FHW[1], HW)
FIELDS = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


def _truth_everywhere(F):
    """In {0, 1}, inside the centre crop, in every frame: EvalEngine keeps every clip."""
    t = np.zeros((F,) + FHW, np.uint8)
    t[:, 30:70, 40:90] = 1
    t[::2, 10:110, 20:40] = 1
    return t


def _truth_early(F):
    """Truth in the frames below 10 only: of a 40-frame video EvalEngine keeps two clips of six."""
    t = _truth_everywhere(F)
    t[10:] = 0
    return t


def _truth_border(F):
    """Everything the centre crop leaves out, and nothing inside it."""
    t = np.ones((F,) + FHW, np.uint8)
    t[:, H0:H0 + HW, W0:W0 + HW] = 0
    return t


def _truth_actors(F):
    """Three actors (1, 2, 3), one value above them (7: "other") and background, moving with the frame."""
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


def _differs(a, b):
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores", "frame_scores") if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    out += [k for k in ("masks", "imap") if not torch.equal(getattr(a, k), getattr(b, k))]
    if a.label != b.label or a.views != b.views:
        out.append("label/views")
    return out


def _tables(ps):
    return [v.table for v in ps.videos]


def _same_tables(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass and score computed once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    kw = dict(instances=K, min_area=MIN_AREA, instance_maps=True)
    de = eng.detect_engine(bs=BS, capacity=64, **kw)
    out = dict(eng=eng, vids=vids, de=de)
    out["first"] = _run(de, vids)
    out["dense"] = [(d.masks.cpu().numpy(), d.imap.cpu().numpy()) for d in out["first"]]
    out["words"] = [r.dev.numel() for r in de.videos]
    out["runs_before"] = de.mask_runs("imap")
    every = [_truth_everywhere(F) for F in FRAMES]
    # a label the detection agrees with, one it does not, one it does
    labels = [out["first"][0].label, (out["first"][1].label + 1) % 24, out["first"][2].label]
    out["every"], out["labels"] = every, labels
    out["score"] = de.score(every, labels)
    out["second_call"] = de.score(every, labels)
    out["actors"] = [_truth_actors(F) for F in FRAMES]
    out["imap_score"] = de.score(out["actors"], labels, actors=ACTORS, which="imap")
    out["after"] = de.results()
    out["runs_after"] = de.mask_runs("imap")
    out["words_after"] = [r.dev.numel() for r in de.videos]
    _run(de, vids)
    out["second_pass"] = de.score(every, labels)
    _run(de, vids, pack=True)
    out["packed"] = de.score(every, labels)
    never = eng.detect_engine(bs=BS, capacity=64, **kw)               # an engine on which the method is never called
    out["never_dets"] = _run(never, vids)
    out["never"] = never
    tf = eng.detect_engine(bs=8, capacity=128, tile=True, flip=True)
    out["tf"] = _run(tf, vids)
    out["tf_engine"] = tf
    return out


def test_tables_are_the_restatement_of_the_engines_own_masks(world):
    ps = world["score"]
    assert isinstance(ps, detect.PassScore) and len(ps.videos) == len(FRAMES) and ps.n_skipped == 0
    fg = 0
    for F, d, (dm, _di), t, lab, v in zip(FRAMES, world["first"], world["dense"], world["every"], world["labels"], ps.videos):
        assert isinstance(v, detect.VideoScore) and v.table.dtype == np.int32 and v.table.shape == (F, 3, 3)
        assert np.array_equal(v.table, ref.crosstab(dm, t, 1, 1))
        assert np.array_equal(v.table.reshape(F, -1).sum(1), np.full(F, FHW[0] * FHW[1]))
        assert np.array_equal(v.counts, ref.seg_counts(dm, t)) and v.counts.dtype == np.int64
        assert np.array_equal(v.table[:, 1:].sum(axis=(1, 2)), d.counts)                    # the predicted pixels are the detection's count
        assert np.array_equal(_bits(v.frame_iou), _bits(v.counts[:, 0] / v.counts[:, 1]))
        assert v.video_iou == v.counts[:, 0].sum() / v.counts[:, 1].sum()
        assert (v.label, v.predicted, v.correct, v.skipped) == (lab, d.label, lab == d.label, False)
        fg += int(v.counts[:, 0].sum())
    assert fg > 0                                                    # the synthetic weights do give foreground on the truth
    assert ps.result["n_correct"] == 2


def test_truth_as_numpy_host_tensor_device_tensor_and_with_a_channel_axis(world):
    de, every, labels = world["de"], world["every"], world["labels"]
    want = _tables(world["packed"])
    forms = [[t[..., None] for t in every], [torch.from_numpy(t) for t in every], [torch.from_numpy(t).cuda() for t in every],
             [torch.from_numpy(t[..., None]).cuda() for t in every]]
    for truths in forms:
        assert _same_tables(_tables(de.score(truths, labels)), want)
    sub = de.score([every[2], every[0], every[2]], [1, 2, 3], videos=[2, 0, 2])
    assert _same_tables(_tables(sub), [want[2], want[0], want[2]]) and [v.label for v in sub.videos] == [1, 2, 3]
    assert de.score([], [], videos=[]).videos == []


def test_the_evaluators_own_tables_with_truth_in_every_clip(world):
    eng, vids, every, labels = world["eng"], world["vids"], world["every"], world["labels"]
    ee = eng.eval_engine(bs=BS, capacity=64)
    want = ee.evaluate(zip(vids, every, labels))
    got = world["score"].result
    assert set(got) == set(want)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind == "f":
            assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a), _bits(b)), k
        else:
            assert np.array_equal(a, b), k
    assert want["n_vids"].sum() == 3 and want["n_tot_frames"].sum() == sum(FRAMES) and want["n_correct"] == 2


def test_truth_free_clips_and_a_video_without_truth(world):
    eng, de, vids, labels = world["eng"], world["de"], world["vids"], world["labels"]
    truths = [_truth_everywhere(1), np.zeros((17,) + FHW, np.uint8), _truth_early(40)]
    ps = de.score(truths, labels)
    assert [v.skipped for v in ps.videos] == [False, True, False] and ps.n_skipped == 1
    assert np.isnan(ps.videos[1].video_iou) and np.isnan(ps.videos[1].frame_iou).all() and not ps.videos[1].correct
    assert np.isnan(ps.videos[2].frame_iou[10:]).all() and not np.isnan(ps.videos[2].frame_iou[:10]).any()
    ee = eng.eval_engine(bs=BS, capacity=64)
    ee.begin()
    assert [ee.add_video(v, t, l) for v, t, l in zip(vids, truths, labels)] == [1, 0, 2]      # the video without truth is skipped there too
    want = ee.results()
    for k in ("frame_ious", "video_ious", "n_tot_frames", "n_vids"):        # n_correct: EvalEngine votes over the two kept clips, the detection over six
        assert np.array_equal(ps.result[k], want[k]), k
    assert want["n_tot_frames"].sum() == 11 and want["n_vids"].sum() == 2


def test_a_tiled_and_mirrored_pass_sees_the_truth_the_crop_leaves_out(world):
    de, tf = world["de"], world["tf_engine"]
    border = [_truth_border(F) for F in FRAMES]
    labels = world["labels"]
    got, centre = tf.score(border, labels), de.score(border, labels)
    inter_tf = inter_c = 0
    for d, t, v, c in zip(world["tf"], border, got.videos, centre.videos):
        assert len(d.views) == 8
        assert np.array_equal(v.table, ref.crosstab(d.masks.cpu().numpy(), t, 1, 1))
        assert not np.array_equal(v.counts, c.counts)
        inter_tf, inter_c = inter_tf + int(v.counts[:, 0].sum()), inter_c + int(c.counts[:, 0].sum())
    print("truth outside the centre crop: intersection %d with tile + flip, %d with the centre crop" % (inter_tf, inter_c))
    assert inter_c == 0 and inter_tf > 0                              # what could not be measured before
    every = tf.score(world["every"], labels)
    for d, t, v in zip(world["tf"], world["every"], every.videos):
        assert np.array_equal(v.table, ref.crosstab(d.masks.cpu().numpy(), t, 1, 1))


def test_maps_of_ranks_against_three_actors(world):
    ps = world["imap_score"]
    ranks = 0
    for F, d, (_dm, di), t, v in zip(FRAMES, world["first"], world["dense"], world["actors"], ps.videos):
        assert v.table.shape == (F, K + 2, ACTORS + 2)
        assert np.array_equal(v.table, ref.crosstab(di, t, K, ACTORS))
        plain = (d.inst_flags & 1) == 0                               # (an overflow frame's map is 255 throughout)
        assert np.array_equal(v.table[plain, 1:K + 1].sum(axis=2), d.inst_areas[plain])      # row r + 1 holds the instance of rank r
        assert v.table[:, :, ACTORS + 1].sum() == (t == 7).sum()
        iou = v.instance_iou()
        assert iou.shape == (F, K, ACTORS) and iou.dtype == np.float64
        for f in (0, F // 2, F - 1):
            for r in range(K):
                for a in range(ACTORS):
                    p, g = di[f] == r + 1, t[f] == a + 1
                    inter, union = int((p & g).sum()), int(p.sum()) + int(g.sum()) - int((p & g).sum())
                    assert iou[f, r, a] == (inter / union if union else 0.0), (f, r, a)
        ranks += int((v.table[:, 1:K + 1, 1:ACTORS + 1] > 0).sum())
    assert ranks > 0                                                 # instances did meet actors
    # the masks of the same pass against the same truth: one foreground slot on the pred side, the same triple
    masks = world["de"].score(world["actors"], world["labels"], actors=ACTORS)
    for m, v in zip(masks.videos, ps.videos):
        assert m.table.shape[1:] == (3, ACTORS + 2) and np.array_equal(m.counts, v.counts)


def test_a_second_call_a_second_pass_and_packing_give_equal_tables(world):
    want = _tables(world["score"])
    for name in ("second_call", "second_pass", "packed"):
        assert _same_tables(_tables(world[name]), want), name
        assert all(np.array_equal(_bits(world[name].result[k]), _bits(world["score"].result[k])) for k in ("fmAP", "vmAP", "accuracy")), name
    assert world["score"].videos[0].table is not world["second_call"].videos[0].table      # arrays of their own, not views of the staging


def test_the_call_changes_no_field_and_no_buffer(world):
    never = world["never"]
    assert world["words"] == world["words_after"] == [r.dev.numel() for r in never.videos]
    assert never.score_ws is None and never.score_pin is None and never.tr_pin == [None, None]      # nothing of it exists until the first call
    for a, b, c in zip(world["first"], world["after"], world["never_dets"]):
        assert _differs(a, b) == [] and _differs(a, c) == []
    for d, (dm, di) in zip(world["after"], world["dense"]):          # the device maps themselves are as they were
        assert np.array_equal(d.masks.cpu().numpy(), dm) and np.array_equal(d.imap.cpu().numpy(), di)
    for a, b in zip(world["runs_before"], world["runs_after"]):
        assert a.shape == b.shape and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.runs, b.runs)


def test_refusals_are_value_errors_before_anything_is_enqueued(world):
    eng, vids = world["eng"], world["vids"]
    fresh = eng.detect_engine(bs=BS, capacity=64, instances=K, instance_maps=True)
    every, labels = world["every"], [0, 1, 2]
    with pytest.raises(ValueError, match="no finished pass"):
        fresh.score(every, labels)
    _run(fresh, vids)
    bad = [(dict(which="mask"), "which"), (dict(which=None), "which"), (dict(actors=0), "actors"), (dict(actors=33), "actors"), (dict(actors=1.5), "actors"),
           (dict(actors="many"), "actors"), (dict(videos=[0, 1, 3]), "video"), (dict(videos=[-1, 0, 1]), "video"), (dict(videos=[0, 1]), "truths"),
           (dict(truths=every[:2]), "truths"), (dict(labels=[0, 1]), "labels"), (dict(labels=[0, 1, 24]), "label"), (dict(labels=[0, -1, 2]), "label"),
           (dict(labels=[0, 1.5, 2]), "label"), (dict(labels=[0, None, 2]), "label"),
           (dict(truths=[every[0], every[1][:16], every[2]]), "shape"), (dict(truths=[every[0], every[1], every[2][:, :, :100]]), "shape"),
           (dict(truths=[every[0], every[1][..., None, None], every[2]]), "shape"), (dict(truths=[every[0], every[1].astype(np.float32), every[2]]), "uint8"),
           (dict(truths=[every[0], every[1].astype(np.int32), every[2]]), "uint8"), (dict(truths=[every[0], every[1].tolist(), every[2]]), "uint8")]
    for kw, word in bad:
        args = dict(truths=every, labels=labels)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            fresh.score(**args)
    assert fresh.score_ws is None and fresh.score_pin is None and fresh.tr_pin == [None, None] and fresh.tr_done == [None, None]      # nothing went up
    records = eng.detect_engine(bs=BS, capacity=64, masks=False)
    _run(records, vids[:1])
    with pytest.raises(ValueError, match="masks=False"):
        records.score(every[:1], [0])
    plain = eng.detect_engine(bs=BS, capacity=64, instances=K)       # no map of ranks kept for the caller
    _run(plain, vids[:1])
    with pytest.raises(ValueError, match="instance_maps"):
        plain.score(every[:1], [0], which="imap")
    assert np.array_equal(plain.score(every[:1], [0]).videos[0].table, world["score"].videos[0].table)
    plain.begin()
    with pytest.raises(ValueError, match="no finished pass"):
        plain.score(every[:1], [0])
    packed = eng.detect_engine(bs=BS, capacity=64)
    packed.begin(True)
    packed.add_video(vids[0])                                        # one clip waits for a full batch: the pass is not finished
    with pytest.raises(ValueError, match="no finished pass"):
        packed.score(every[:1], [0])
    packed.results()
    assert np.array_equal(packed.score(every[:1], [0]).videos[0].table, world["score"].videos[0].table)


def test_a_pass_and_score_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with both scores on the step engine's weights, train step, against the same two steps on a fresh engine: the
    second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are equal bit for
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
            for which, P in (("masks", 1), ("imap", K)):
                ps = de.score(world["actors"][:2], [0, 1], actors=ACTORS, which=which)
                for d, t, v in zip(dets, world["actors"], ps.videos):
                    assert np.array_equal(v.table, ref.crosstab(getattr(d, which).cpu().numpy(), t, P, ACTORS))
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
