"""GPU: truth given as evalstep.BoxTruth through the engines, at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as
tests/test_detect_recut_gpu.py is sized (the tile + flip engine takes bs = 8).  EvalEngine over the synthetic box videos equals EvalEngine
over their dense(binary=True) in every key, clip count and skip, packed or not, whatever the rects' values; a warm add_video with boxes makes
no host wait but for its upload slot of two videos ago, where the dense path makes one per video; DetectEngine.score and sweep with box truths
equal the calls with their dense() bit for bit -- masks, maps of ranks with actors, a video without a box, dense and box truths mixed, a tiled
and mirrored pass --; refusals are ValueErrors that enqueue nothing; a pass plus score with boxes between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, step as pstep, synthetic
from picons_amd.evalstep import BoxTruth

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
K, MIN_AREA = 8, 3


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


def _moving(F, x, y, w, h, dx=1, dy=1):
    return [[x + dx * f, y + dy * f, w, h] for f in range(F)]


def _box_truths():
    """Per video of FRAMES: one actor in every frame; NO box at all; two overlapping actors over different frame ranges."""
    H, W = FHW
    a = BoxTruth.from_annotation((0, 0, 0, _moving(1, 40, 30, 50, 40), [0]), 1, H, W)
    none = BoxTruth((17, H, W), np.zeros((17, 1, 5), np.int32))
    two = BoxTruth.from_annotations([(0, 30, 0, _moving(31, 20, 10, 60, 70), [0]), (5, 60, 0, _moving(35, 50, 40, 70, 60, dx=-1, dy=0), [7])], 40, H, W)
    return [a, none, two]


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _same_result(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k
        assert x.tobytes() == y.tobytes(), k                        # bit for bit, NaNs in the same places


def _same_scores(a, b):
    assert len(a.videos) == len(b.videos) and a.n_skipped == b.n_skipped
    for x, y in zip(a.videos, b.videos):
        assert x.table.dtype == y.table.dtype and np.array_equal(x.table, y.table)
        assert (x.label, x.predicted, x.correct, x.skipped) == (y.label, y.predicted, y.correct, y.skipped)
    _same_result(a.result, b.result)


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2), the synthetic evaluation set both ways, a detection pass with maps of ranks and probabilities kept, its dense
    scores: computed once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    kw = dict(hw=HW, frames_hw=FHW)
    boxes = synthetic.make_eval_videos_boxes(4, **kw)
    dense = [(f, t.dense(binary=True), lab) for f, t, lab in boxes]
    for (fa, ta, la), (fb, tb, lb) in zip(synthetic.make_eval_videos_u8(4, **kw), dense):
        assert np.array_equal(fa, fb) and np.array_equal(ta[..., 0], tb) and la == lb
    vids = _videos()
    de = eng.detect_engine(bs=BS, capacity=64, instances=K, min_area=MIN_AREA, instance_maps=True)
    de.set_keep_probs(True)
    dets = _run(de, vids)
    truths = _box_truths()
    labels = [dets[0].label, (dets[1].label + 1) % 24, dets[2].label]
    out = dict(eng=eng, boxes=boxes, dense=dense, vids=vids, de=de, truths=truths, labels=labels)
    out["dense_truths"] = [t.dense() for t in truths]
    out["score_dense"] = de.score(out["dense_truths"], labels)
    return out


# ---------------------------------------------------------------------- EvalEngine
@pytest.mark.parametrize("pack", [False, True])
def test_eval_engine_with_boxes_equals_the_dense_pass(world, pack):
    ee = world["eng"].eval_engine(bs=BS, capacity=64)
    res, counts, skipped = [], [], []
    for vids in (world["dense"], world["boxes"]):
        ee.begin(pack)
        counts.append([ee.add_video(f, t, lab) for f, t, lab in vids])
        res.append(ee.results())
        skipped.append((ee.n_videos, ee.n_skipped, ee.n_clips))
    assert counts[0] == counts[1] and counts[0][1] == 0 and all(c > 0 for i, c in enumerate(counts[0]) if i != 1)
    assert skipped[0] == skipped[1] and skipped[0][1] == 1
    _same_result(res[0], res[1])
    _same_result(ee.evaluate(world["boxes"], pack=pack), res[0])     # and through evaluate(), boxes after boxes on warm slots


def test_eval_engine_paints_binary_whatever_the_values(world):
    ee = world["eng"].eval_engine(bs=BS, capacity=64)
    valued = []
    for f, t, lab in world["boxes"]:
        r = t.rects.copy()
        r[:, 0, 4] *= 3
        r[:, 1, 4] *= 7
        valued.append((f, BoxTruth(t.shape, r), lab))
    assert set(np.unique(valued[0][1].dense())) == {0, 3, 7}
    assert np.array_equal(valued[0][1].dense(binary=True), world["dense"][0][1])
    _same_result(ee.evaluate(valued), ee.evaluate(world["dense"]))
    # frames already on the device: the map is painted into a buffer of its own
    on_dev = [(torch.from_numpy(f).cuda(), t, lab) for f, t, lab in valued]
    _same_result(ee.evaluate(on_dev), ee.evaluate(world["dense"]))


def test_a_warm_add_video_with_boxes_does_not_wait(world, monkeypatch):
    ee = world["eng"].eval_engine(bs=BS, capacity=64)
    three = [world["boxes"][i] for i in (0, 2, 3)]
    three_dense = [world["dense"][i] for i in (0, 2, 3)]
    ee.evaluate(three)                                               # warm: pool, slots and tables exist
    calls = []
    for cls, name in ((torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize")):
        real = getattr(cls, name)
        monkeypatch.setattr(cls, name, (lambda real, tag: lambda *a, **k: (calls.append(tag), real(*a, **k))[1])(real, "%s.%s" % (cls.__name__, name)))
    ee.begin()
    for f, t, lab in three:
        assert ee.add_video(f, t, lab) > 0
    waits_boxes = list(calls)
    assert len(waits_boxes) <= 1, waits_boxes                        # at most its own upload slot, two videos back, for the third video
    boxes_result = ee.results()
    del calls[:]
    ee.begin()
    for f, t, lab in three_dense:
        assert ee.add_video(f, t, lab) > 0
    waits_dense = list(calls)
    assert len(waits_dense) == 3 and all(w == "Event.synchronize" for w in waits_dense)        # the dense path: one per video
    monkeypatch.undo()
    _same_result(boxes_result, ee.results())
    print("host waits over three videos: boxes %s, dense %s" % (waits_boxes, waits_dense))


# ---------------------------------------------------------------------- DetectEngine.score / sweep
def test_score_with_boxes_equals_score_with_their_dense_maps(world):
    de, truths, labels = world["de"], world["truths"], world["labels"]
    want = world["score_dense"]
    got = de.score(truths, labels)
    _same_scores(got, want)
    assert want.videos[0].table.shape == (1, 3, 3) and want.videos[0].table[:, :, 1:].sum() == 50 * 40
    assert want.videos[1].table[:, :, 1:].sum() == 0 and want.n_skipped >= 1 and want.videos[1].skipped            # the video without any box
    assert want.videos[2].table[:, :, 1:].sum() == int((world["dense_truths"][2] != 0).sum()) > 0
    # one call of dense and box truths mixed, host and device
    mixed = [truths[0], torch.from_numpy(world["dense_truths"][1]).cuda(), truths[2]]
    _same_scores(de.score(mixed, labels), want)
    _same_scores(de.score([world["dense_truths"][0], truths[1], world["dense_truths"][2][..., None]], labels), want)
    # picked videos
    one = de.score([truths[2]], [labels[2]], videos=[2])
    assert np.array_equal(one.videos[0].table, want.videos[2].table)


def test_the_values_carry_the_actors_into_the_map_of_ranks_score(world):
    de, truths, labels = world["de"], world["truths"], world["labels"]
    d2 = world["dense_truths"][2]
    assert set(np.unique(d2)) == {0, 1, 2} and (d2[10] == 2).any() and (d2[10] == 1).any()       # two actors that overlap: the later one on top
    want = de.score(world["dense_truths"], labels, actors=2, which="imap")
    got = de.score(truths, labels, actors=2, which="imap")
    _same_scores(got, want)
    assert got.videos[2].table.shape == (40, K + 2, 4)
    assert got.videos[2].table[:, :, 1].sum() == int((d2 == 1).sum()) and got.videos[2].table[:, :, 2].sum() == int((d2 == 2).sum())
    # a value above `actors` lands in slot A + 1, as a dense byte would
    _same_scores(de.score(truths, labels, actors=1, which="imap"), de.score(world["dense_truths"], labels, actors=1, which="imap"))
    assert de.score(truths, labels, actors=1, which="imap").videos[2].table[:, :, 2].sum() == int((d2 == 2).sum())


def test_score_under_tile_and_flip(world):
    tf = world["eng"].detect_engine(bs=8, capacity=128, tile=True, flip=True)
    _run(tf, world["vids"])
    _same_scores(tf.score(world["truths"], world["labels"]), tf.score(world["dense_truths"], world["labels"]))


def test_sweep_with_boxes_equals_sweep_with_their_dense_maps(world):
    de, truths, labels = world["de"], world["truths"], world["labels"]
    want = de.sweep(world["dense_truths"], labels)
    got = de.sweep(truths, labels)
    assert np.array_equal(got.words, want.words) and len(got.results) == len(want.results) == 19 and got.n_skipped == want.n_skipped
    for a, b in zip(got.videos, want.videos):
        assert np.array_equal(a, b)
    for a, b in zip(got.results, want.results):
        _same_result(a, b)
    assert sum(int(h[:, 1].sum()) for h in want.videos) == sum(int((t != 0).sum()) for t in world["dense_truths"])


def test_refusals_are_value_errors_and_enqueue_nothing(world):
    de, truths, labels = world["de"], world["truths"], world["labels"]
    H, W = FHW
    slot, done, bslot, bdone = de.tr_slot, list(de.tr_done), de.bx_slot, list(de.bx_done)
    wrong_shape = BoxTruth((40, H, W + 1), np.zeros((40, 1, 5), np.int32))
    too_many = BoxTruth((40, H, W), np.zeros((40, 1, 5), np.int32))
    too_many.rects = np.zeros((40, 33, 5), np.int32)                 # (the constructor refuses R = 33 itself)
    for call in (de.score, de.sweep):
        with pytest.raises(ValueError, match="truth of video 2 has shape"):
            call([truths[0], truths[1], wrong_shape], labels)
        with pytest.raises(ValueError, match="R in 1..32"):
            call([truths[0], truths[1], too_many], labels)
        with pytest.raises(ValueError, match="2 truths and 3 labels for 3 videos"):
            call(truths[:2], labels)
        with pytest.raises(ValueError, match="truth of video 0 has shape"):
            call([truths[2]], [labels[0]], videos=[0])
    with pytest.raises(ValueError, match="BoxTruth"):
        BoxTruth((40, H, W), np.zeros((40, 33, 5), np.int32))
    assert de.tr_slot == slot and all(a is b for a, b in zip(de.tr_done, done))                  # no upload slot was taken,
    assert de.bx_slot == bslot and all(a is b for a, b in zip(de.bx_done, bdone))                # of the dense truths' or of the tables'
    ee = world["eng"].eval_engine(bs=BS, capacity=64)
    ee.begin()
    f = world["boxes"][0][0]
    for bad in (wrong_shape, BoxTruth((f.shape[0] + 1, H, W), np.zeros((f.shape[0] + 1, 1, 5), np.int32))):
        with pytest.raises(ValueError, match="add_video: truth has shape"):
            ee.add_video(f, bad, 0)
    assert ee.n_videos == 0 and ee.n_skipped == 0 and ee.pool == [] and ee.up_done == [None, None]
    _same_scores(de.score(truths, labels), world["score_dense"])     # a following score still works and equals the earlier one


def test_a_pass_and_a_score_with_boxes_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass plus score with box truths and an EvalEngine pass with boxes on the step engine's weights, train step,
    against the same two steps on a fresh engine: the second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running
    statistics and the step count are equal bit for bit."""
    eng, de = world["eng"], world["de"]
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            _run(de, world["vids"])
            _same_scores(de.score(world["truths"], world["labels"]), de.score(world["dense_truths"], world["labels"]))
            ee = eng.eval_engine(bs=BS, capacity=64)
            _same_result(ee.evaluate(world["boxes"][:2]), ee.evaluate(world["dense"][:2]))
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
