"""GPU: detect.DetectEngine.set_clip_hop at hw = 112, frames of 120 x 136 and synthetic weights, the setup of tests/test_detect_views_gpu.py.
Videos of 17, 33 and 40 frames at hop 8 and hop 4: masks, counts and boxes are exact against the numpy restatement (tests/clip_hop_ref.py on
tests/detectviews_ref.Merge, then tests/resample_ref.py) applied to the engine's OWN logits, captured per batch through on_batch; label and
class scores are evalstep.vote over all rows of all overlapping clips; packing, another batch size and a second pass change no bit;
set_clip_hop(16) and set_clip_hop(None) are an engine that never called it; tile + flip and a working frame; instances, instance scores,
links, row runs and score() work behind it unchanged; a refused hop or video changes nothing; a pass between two train steps changes
nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, ops, step as pstep, synthetic
from tests import clip_hop_ref as hop_ref, map_crosstab_ref, resample_ref as ref

pytestmark = pytest.mark.gpu
HW, FS = 112, 2
NATIVE, WORK = (120, 136), (128, 144)
FRAMES = (17, 33, 40)
K = 4


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos(hw, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (F,) + hw + (3,), dtype=np.uint8) for F in FRAMES]


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _differs(a, b):
    """The fields in which two detections differ (bit for bit), as a list of names: empty if they are the same."""
    bits = lambda x: np.asarray(x, np.float32).view(np.int32)
    eq = dict(label=a.label == b.label, class_score=np.array_equal(bits(a.class_score), bits(b.class_score)),
              class_scores=np.array_equal(bits(a.class_scores), bits(b.class_scores)), counts=np.array_equal(a.counts, b.counts),
              boxes=np.array_equal(a.boxes, b.boxes), frame_scores=np.array_equal(bits(a.frame_scores), bits(b.frame_scores)),
              masks=torch.equal(a.masks, b.masks), views=a.views == b.views, hop=a.hop == b.hop)
    return [k for k, v in eq.items() if not v]


def _recorded(eng, vids, hop, bs, capacity=64, work=None, **kw):
    """A pass at `hop` with every batch's logits and class scores kept -> (engine, detections, [(m, logits, scores)])."""
    rec = []
    de = eng.detect_engine(bs=bs, capacity=capacity, on_batch=lambda m, lg, sc: rec.append((m, lg.cpu().numpy(), sc.cpu().numpy())), **kw)
    if work:
        de.set_working_frame(work, "area")
    de.set_clip_hop(hop)
    dets = _run(de, vids)
    de.on_batch = None
    return de, dets, rec


def _check_against_restatement(vids, dets, rec, hop, bs, views, frame):
    """pack=False: a video's clips come in batches of bs // V of its own.  The restatement on the recorded logits -> masks, counts, boxes exact,
    the scores within the bar of the scaled tests, label and class scores the vote over all rows; -> (positive, all) pixels."""
    V, per, it = len(views), bs // len(views), iter(rec)
    npos = ntot = 0
    for frames, det in zip(vids, dets):
        F, H, W = frames.shape[:3]
        starts = detect.clip_starts_hop(F, FS, hop)
        xs, rows = [], []
        for i in range(0, len(starts), per):
            n = min(per, len(starts) - i)
            m, lg, sc = next(it)
            assert m == n * V and lg.shape == (m, 1, 8, HW, HW) and sc.shape == (m, 24)
            xs.append(lg[:, 0].reshape(V, n, 8, HW, HW))
            rows += [sc[v * n + c] for c in range(n) for v in range(V)]                    # ring order: row0 + clip * V + view
        _per, num, mean = hop_ref.restate(np.concatenate(xs, axis=1), starts, F, FS, hop, views, frame[0], frame[1], HW)
        v, covered = ref.resample(mean, np.broadcast_to(num, mean.shape), H, W)
        exp = ref.masks(v, covered)
        masks = det.masks.cpu().numpy()
        assert masks.shape == (F, H, W) and masks.dtype == np.uint8 and np.array_equal(masks, exp), (F, hop)
        assert det.views == views and det.hop == hop and det.counts.shape == (F,) and det.boxes.shape == (F, 4)
        for f in range(F):
            cnt = int(exp[f].sum())
            assert det.counts[f] == cnt and tuple(det.boxes[f]) == ref.box_of(exp[f]), (F, f)
            if cnt == 0:
                assert det.frame_scores[f] == 0.0
                continue
            r64, r32 = ref.score_refs(v[f], exp[f])
            assert abs(float(det.frame_scores[f]) - r64) <= max(1e-6, 2.0 * abs(r32 - r64)), (F, f, det.frame_scores[f], r64, r32)
        npos += int(exp.sum()); ntot += exp.size
        scores = np.stack(rows)
        assert scores.shape == (len(starts) * V, 24) and det.label == evalstep.vote(scores)
        mean_scores = scores[0].copy()
        for r in scores[1:]:
            mean_scores = (mean_scores + r).astype(np.float32)
        mean_scores = (mean_scores / np.float32(len(scores))).astype(np.float32)
        assert np.array_equal(det.class_scores.view(np.int32), mean_scores.view(np.int32)) and det.class_score == mean_scores[det.label]
    assert next(it, None) is None
    return npos, ntot


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2), the videos, and the plain centre-crop pass every other pass is held against.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos(NATIVE, 41)
    plain = eng.detect_engine(bs=4, capacity=64)
    return dict(eng=eng, vids=vids, plain=plain, base=_run(plain, vids))


@pytest.mark.parametrize("hop", [8, 4])
def test_detections_equal_a_numpy_restatement_of_the_engines_own_logits(world, hop):
    eng, vids = world["eng"], world["vids"]
    views = [evalstep.centre_crop(*NATIVE, HW) + (0,)]
    de, dets, rec = _recorded(eng, vids, hop, bs=4)
    assert [len(r.starts) for r in de.videos] == [len(detect.clip_starts_hop(F, FS, hop)) for F in FRAMES] and all(r.planes is None for r in de.videos)
    npos, ntot = _check_against_restatement(vids, dets, rec, hop, 4, views, NATIVE)
    print("clip hop engine, hop %d: %d of %d pixels positive" % (hop, npos, ntot))
    assert 0 < npos < ntot
    # pack on, another batch size, a second pass: the same detections bit for bit
    other = eng.detect_engine(bs=3, capacity=64)
    other.set_clip_hop(hop)
    for again in (_run(de, vids), _run(de, vids, pack=True), _run(other, vids), _run(other, vids, pack=True)):
        assert [_differs(a, b) for a, b in zip(dets, again)] == [[]] * len(vids)
    assert any(_differs(a, b) for a, b in zip(dets, world["base"]))           # and not those of today's cut


def test_the_full_span_and_none_are_an_engine_that_never_called_it(world):
    eng, vids, base = world["eng"], world["vids"], world["base"]
    de = eng.detect_engine(bs=4, capacity=64)
    for hop in (16, None):
        de.set_clip_hop(4)
        de.set_clip_hop(hop)
        got = _run(de, vids)
        assert [_differs(a, b) for a, b in zip(base, got)] == [[]] * len(vids) and all(d.hop is None for d in got)
        assert de.ws_planes is None and all(r.planes is None and r.hop is None for r in de.videos)
        assert [r.dev.numel() for r in de.videos] == [r.dev.numel() for r in world["plain"].videos]
    # a video keeps the hop it was added under
    de.begin()
    de.set_clip_hop(8)
    de.add_video(vids[1])
    de.set_clip_hop(None)
    de.add_video(vids[1])
    mixed = de.results()
    assert (mixed[0].hop, mixed[1].hop) == (8, None) and _differs(mixed[1], base[1]) == [] and "masks" in _differs(mixed[0], mixed[1])


@pytest.mark.parametrize("work", [None, WORK], ids=["tile_flip", "tile_flip_working_frame"])
def test_with_tile_and_flip_and_on_a_working_frame(world, work):
    eng, vids, hop = world["eng"], world["vids"][:2], 8
    frame = work or NATIVE
    views = detect.make_views(frame[0], frame[1], HW, True, True)
    assert len(views) == 8
    de, dets, rec = _recorded(eng, vids, hop, bs=8, capacity=96, work=work, tile=True, flip=True)
    npos, ntot = _check_against_restatement(vids, dets, rec, hop, 8, views, frame)
    assert 0 < npos < ntot and all(d.work == (work + ("area",) if work else None) and d.masks.shape[1:] == NATIVE for d in dets)
    assert [_differs(a, b) for a, b in zip(dets, _run(de, vids, pack=True))] == [[]] * len(vids)


def test_instances_scores_links_runs_and_score_work_behind_it(world):
    eng, vids, hop = world["eng"], world["vids"], 4
    de = eng.detect_engine(bs=4, capacity=64, instances=K, instance_maps=True, instance_scores=True, instance_links=1)
    de.set_clip_hop(hop)
    dets = _run(de, vids)
    plain = eng.detect_engine(bs=4, capacity=64)
    plain.set_clip_hop(hop)
    truths = []
    for frames, d, base in zip(vids, dets, _run(plain, vids)):
        F, H, W = frames.shape[:3]
        assert _differs(d, base) == []                                  # the options change nothing the plain pass leaves
        masks, imap = d.masks.cpu().numpy(), d.imap.cpu().numpy()
        inst, want_map = ops.frame_instances(d.masks, conn=8, min_area=1, K=K)
        n, kept, _runs, flags, areas, ibox, first = ops.decode_instances(inst.cpu().numpy(), K)
        n, kept, flags, areas, ibox, first = detect.substitute_overflow(d.counts, d.boxes, 1, (n, kept, flags, areas, ibox, first))
        for got, want in ((d.inst_n, n), (d.inst_kept, kept), (d.inst_flags, flags), (d.inst_areas, areas), (d.inst_boxes, ibox), (d.inst_first, first)):
            assert np.array_equal(got, want)
        assert np.array_equal(imap, want_map.cpu().numpy()) and np.array_equal(imap != 0, masks != 0)
        assert d.inst_scores.shape == (F, K) and d.inst_overlaps.shape == (F, 1, K + 1, K + 1) and d.probs.shape == (F, H, W)
        probs = d.probs.cpu().numpy().view(np.uint16)
        assert ((probs >= 32768) | (masks == 0)).all() and int(d.inst_kept.sum()) > 0      # a positive pixel has probability >= 0.5
        t = np.zeros((F, H, W), np.uint8)
        t[:, 20:70, 30:120] = 1
        t[::2, 5:85, 10:40] = 2
        truths.append(t)
    for d, r in zip(dets, de.mask_runs()):
        assert np.array_equal(r.dense(), d.masks.cpu().numpy())
    ps = de.score(truths, [d.label for d in dets], actors=2)
    for d, t, vs in zip(dets, truths, ps.videos):
        m = d.masks.cpu().numpy()
        assert np.array_equal(vs.table, map_crosstab_ref.crosstab(m, t, 1, 2)) and vs.correct
        inter, union, gt = ((m != 0) & (t != 0)), ((m != 0) | (t != 0)), t != 0
        assert np.array_equal(vs.counts, np.stack([x.reshape(len(m), -1).sum(1) for x in (inter, union, gt)], axis=1))


def test_a_refused_hop_or_video_changes_nothing(world):
    eng, vids = world["eng"], world["vids"]
    de = eng.detect_engine(bs=4, capacity=11)                           # capacity - bs = 7 rows for a video
    de.set_clip_hop(8)
    want = _run(de, vids[:1])                                           # 17 frames at hop 8: 4 clips
    for hop in (0, 3, 18, 4.0, True, "8"):
        with pytest.raises(ValueError, match="set_clip_hop"):
            de.set_clip_hop(hop)
        assert de.hop == 8
    de.begin()
    de.add_video(vids[0])
    pos, n = de.pos, len(de.videos)
    with pytest.raises(ValueError, match="hop = 8"):
        de.add_video(vids[2])                                           # 40 frames at hop 8: 8 clips
    de.set_clip_hop(4)
    with pytest.raises(ValueError, match="hop = 4"):
        de.add_video(vids[1])                                           # 33 frames at hop 4: 12 clips
    with pytest.raises(ValueError):
        de.add_video(vids[0][:, :100])                                  # smaller than the crop
    assert (de.pos, len(de.videos)) == (pos, n)
    assert _differs(de.results()[0], want[0]) == []


def test_a_hopped_pass_between_two_train_steps_changes_nothing(world):
    """Train step, hopped detection pass on the step engine's weights, train step, against the same two steps on a fresh engine: the second
    step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are equal bit for bit."""
    eng = world["eng"]
    de = eng.detect_engine(bs=4, capacity=64)
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            de.set_clip_hop(4)
            dets = _run(de, world["vids"][:2])
            assert all(d.hop == 4 and d.masks.shape[1:] == NATIVE for d in dets)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
