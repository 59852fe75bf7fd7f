"""GPU: detect.DetectEngine.set_working_frame at hw = 112, bs = 8 and synthetic weights, the setup of tests/test_detect_views_gpu.py.  A working
frame of the video's own size gives today's detections bit for bit; videos of 90 x 160 resized to 120 x 136 ("area") give masks, counts and
boxes that are exact against the numpy restatement (tests/resample_ref.py on tests/detectviews_ref.Merge) of the engine's OWN logits, at
native size; a video smaller than the crop is taken; instances, instance scores, links, row runs and score() work behind it unchanged;
packing, a second pass and the switch back; a pass between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, ops, step as pstep, synthetic
from tests import map_crosstab_ref, resample_ref as ref

pytestmark = pytest.mark.gpu
HW, BS = 112, 8
WORK, NATIVE, SMALL = (120, 136), (90, 160), (60, 80)
FRAMES = (1, 17, 40)
K = 8


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
              masks=torch.equal(a.masks, b.masks), views=a.views == b.views)
    return [k for k, v in eq.items() if not v]


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass computed once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos(NATIVE, 29)
    out = dict(eng=eng, vids=vids)
    for name, kw in (("tile_flip", dict(tile=True, flip=True)), ("tile", dict(tile=True))):
        rec, resized = [], []
        de = eng.detect_engine(bs=BS, capacity=64, **kw)

        def hook(m, lg, sc, de=de, rec=rec, resized=resized):
            rec.append((m, lg.cpu().numpy(), sc.cpu().numpy()))
            r = de.videos[-1]                                            # the video whose clips run: while more of them wait, upload and working video live
            if r.video is not None and r.wvideo is not None:
                resized.append((len(de.videos) - 1, r.video.cpu().numpy(), r.wvideo.cpu().numpy(),
                                ops.resize_u8(r.video, WORK[0], WORK[1], 3).cpu().numpy()))
        de.on_batch = hook
        de.set_working_frame(WORK, "area")
        first = _run(de, vids)
        de.on_batch = None
        out[name] = dict(de=de, rec=rec, resized=resized, first=first, words=[r.dev.numel() for r in de.videos], again=_run(de, vids),
                         packed=_run(de, vids, pack=True))
    return out


@pytest.mark.parametrize("kw", [dict(), dict(tile=True, flip=True)], ids=["centre", "tile_flip"])
def test_a_working_frame_of_the_videos_own_size_changes_no_bit(world, kw):
    eng, vids = world["eng"], _videos(WORK, 31)
    plain, same = eng.detect_engine(bs=BS, capacity=64, **kw), eng.detect_engine(bs=BS, capacity=64, **kw)
    same.set_working_frame(WORK)
    a, b = _run(plain, vids), _run(same, vids)
    assert [_differs(x, y) for x, y in zip(a, b)] == [[]] * len(vids)
    assert [r.dev.numel() for r in plain.videos] == [r.dev.numel() for r in same.videos]
    assert all(d.work is None for d in a) and all(d.work == WORK + ("area",) for d in b)
    assert plain.ws_scaled is None and same.ws_scaled is not None and same.ws_views is None
    assert 0 < sum(int(d.counts.sum()) for d in a) < sum(d.masks.numel() for d in a)


@pytest.mark.parametrize("name,tile,flip", [("tile_flip", True, True), ("tile", True, False)])
def test_detections_at_native_size_equal_a_numpy_restatement_of_the_engines_own_logits(world, name, tile, flip):
    w = world[name]
    views = detect.make_views(WORK[0], WORK[1], HW, tile, flip)        # of the WORKING frame
    V = len(views)
    assert V == (8 if flip else 4) and views[-1][:2] == (8, 24)
    # the working video is ops.resize_u8 of the upload, and the upload the video
    assert 2 in {i for i, _u, _w, _r in w["resized"]}              # the 40-frame video: clips still wait while its first run
    for i, up, work, want in w["resized"]:
        assert np.array_equal(up, world["vids"][i]) and work.shape == (FRAMES[i],) + WORK + (3,) and np.array_equal(work, want)
    it = iter(w["rec"])
    per = BS // V
    npos = ntot = 0
    for frames, det in zip(world["vids"], w["first"]):
        F, H, W = frames.shape[:3]
        assert (H, W) == NATIVE
        starts = evalstep.clip_starts(F, np.ones(F))
        merge, rows = ref.Merge(F, WORK[0], WORK[1], HW), []
        for i in range(0, len(starts), per):
            n = min(per, len(starts) - i)
            m, lg, sc = next(it)
            assert m == n * V and lg.shape == (m, 1, 8, HW, HW) and sc.shape == (m, 24)
            merge.add(lg[:, 0].reshape(V, n, 8, HW, HW), views, starts[i:i + n])
            rows += [sc[v * n + c] for c in range(n) for v in range(V)]                    # ring order: row0 + clip * V + view
        assert (merge.num >= 1).all()
        v, covered = ref.resample(merge.merged(), merge.num, H, W)
        exp = ref.masks(v, covered)
        masks = det.masks.cpu().numpy()
        assert masks.shape == (F, H, W) and masks.dtype == np.uint8 and np.array_equal(masks, exp)
        assert det.views == views and det.work == WORK + ("area",) and det.counts.shape == (F,) and det.boxes.shape == (F, 4)
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
    assert next(it, None) is None
    print("scaled detect engine, %s: %d of %d native pixels positive" % (name, npos, ntot))
    assert 0 < npos < ntot                                             # the masks are neither empty nor full: the comparison means something


def test_a_video_smaller_than_the_crop_is_taken_on_a_working_frame(world):
    eng, vids = world["eng"], _videos(SMALL, 37)
    de = eng.detect_engine(bs=BS, capacity=64)
    with pytest.raises(ValueError, match="smaller"):
        de.detect(vids[1])
    de.set_working_frame((HW, HW), "linear")
    dets = _run(de, vids)
    for F, d in zip(FRAMES, dets):
        assert d.masks.shape == (F,) + SMALL and d.views == [(0, 0, 0)] and d.work == (HW, HW, "linear") and d.counts.shape == (F,)
        m = d.masks.cpu().numpy()
        assert np.array_equal(m.reshape(F, -1).sum(1), d.counts) and all(tuple(d.boxes[f]) == ref.box_of(m[f]) for f in range(F))
    de.set_working_frame(None)
    with pytest.raises(ValueError, match="smaller"):
        de.detect(vids[1])


def test_instances_scores_links_runs_and_score_work_behind_it(world):
    eng, vids = world["eng"], world["vids"]
    rec = []
    de = eng.detect_engine(bs=BS, capacity=64, tile=True, flip=True, instances=K, instance_maps=True, instance_scores=True, instance_links=2,
                           on_batch=lambda m, lg, sc: rec.append(lg.cpu().numpy()))
    de.set_working_frame(WORK, "area")
    dets = _run(de, vids)
    de.on_batch = None
    views = detect.make_views(WORK[0], WORK[1], HW, True, True)
    it = iter(rec)
    truths = []
    for frames, d, base in zip(vids, dets, world["tile_flip"]["first"]):
        F, H, W = frames.shape[:3]
        assert _differs(d, base) == []                                  # the options change nothing the plain pass leaves
        masks, imap = d.masks.cpu().numpy(), d.imap.cpu().numpy()
        assert imap.shape == (F, H, W) and d.inst_overlaps.shape == (F, 2, K + 1, K + 1) and d.inst_scores.shape == (F, K)
        over = (d.inst_flags & 1) != 0
        other = (imap == 255).reshape(F, -1).sum(1)
        assert np.array_equal((d.inst_areas.sum(1) + other)[~over], d.counts[~over]) and np.array_equal((imap != 0), masks != 0)
        assert np.array_equal(d.inst_areas[over, 0], d.counts[over])
        merge = ref.Merge(F, WORK[0], WORK[1], HW)
        for s in evalstep.clip_starts(F, np.ones(F)):
            merge.add(next(it)[:, 0].reshape(8, 1, 8, HW, HW), views, [s])
        v, covered = ref.resample(merge.merged(), merge.num, H, W)
        probs = d.probs.cpu().numpy().view(np.uint16)
        assert probs.shape == (F, H, W) and np.array_equal(probs, ref.expected_probs(v, covered))
        t = np.zeros((F, H, W), np.uint8)
        t[:, 20:70, 30:120] = 1
        t[::2, 5:85, 10:40] = 2
        truths.append(t)
    assert next(it, None) is None
    for d, r in zip(dets, de.mask_runs()):
        assert np.array_equal(r.dense(), d.masks.cpu().numpy())
    for d, r in zip(dets, de.mask_runs("imap")):
        assert np.array_equal(r.dense(), d.imap.cpu().numpy())
    ps = de.score(truths, [d.label for d in dets], actors=2)
    for d, t, vs in zip(dets, truths, ps.videos):
        assert np.array_equal(vs.table, map_crosstab_ref.crosstab(d.masks.cpu().numpy(), t, 1, 2)) and vs.correct
    ps = de.score(truths, [d.label for d in dets], actors=2, which="imap")
    for d, t, vs in zip(dets, truths, ps.videos):
        assert np.array_equal(vs.table, map_crosstab_ref.crosstab(d.imap.cpu().numpy(), t, K, 2))
    with pytest.raises(ValueError, match="shape"):
        de.score([np.zeros((F,) + WORK, np.uint8) for F in FRAMES], [0, 0, 0])          # the truth is native, not working size


@pytest.mark.parametrize("name", ["tile_flip", "tile"])
def test_packing_a_second_pass_and_the_switch_back(world, name):
    w = world[name]
    assert [d.counts.size for d in w["first"]] == list(FRAMES)
    for other in ("again", "packed"):
        assert [_differs(a, b) for a, b in zip(w["first"], w[other])] == [[]] * len(FRAMES), (name, other)
    if name == "tile":
        return
    # back to the videos' own scale between passes: today's path, bit for bit, on the same engine; and forth again
    eng, de = world["eng"], w["de"]
    own = _videos(WORK, 31)
    want = _run(eng.detect_engine(bs=BS, capacity=64, tile=True, flip=True), own)
    de.set_working_frame(None)
    got = _run(de, own)
    assert [_differs(a, b) for a, b in zip(want, got)] == [[]] * len(own) and all(d.work is None for d in got)
    assert [r.dev.numel() for r in de.videos] == w["words"]
    de.set_working_frame(WORK, "area")
    assert [_differs(a, b) for a, b in zip(w["first"], _run(de, world["vids"]))] == [[]] * len(FRAMES)
    # a video keeps the working frame it was added under
    de.begin()
    de.add_video(world["vids"][1])
    de.set_working_frame(None)
    de.add_video(own[1])
    mixed = de.results()
    assert _differs(mixed[0], w["first"][1]) == [] and _differs(mixed[1], want[1]) == [] and (mixed[0].work, mixed[1].work) == (WORK + ("area",), None)


def test_a_scaled_pass_between_two_train_steps_changes_nothing(world):
    """Train step, scaled detection pass on the step engine's weights, train step, against the same two steps on a fresh engine: the second
    step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are equal bit for bit."""
    eng, de = world["eng"], world["tile_flip"]["de"]
    fresh = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, between in ((eng, True), (fresh, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if between:
            de.set_working_frame(WORK, "area")
            dets = _run(de, world["vids"][:2])
            assert all(d.work == WORK + ("area",) and d.masks.shape[1:] == NATIVE for d in dets)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
