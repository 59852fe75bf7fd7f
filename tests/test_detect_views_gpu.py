"""GPU: detect.DetectEngine with views (tile / flip) at hw = 112 with frames of 120 x 136 -- tiles at h0 in {0, 8}, w0 in {0, 24} -- bs = 8 and
synthetic weights.  tile + flip: V = 8 views, one clip per batch; tile alone: V = 4, two clips per batch.  The per-view logits come through
on_batch (a segment of n clips lies view-major: view v of its clip c at slot v * n + c); masks, counts and boxes must be exact against the
numpy restatement (tests/detectviews_ref.py) of the engine's OWN logits, the class against evalstep.vote over the clips * V score rows in
ring order (row0 + clip * V + view).  Also: the ways of batching and a second pass, the two refusals, the default path left as it is, and
the direction of the un-flip (a left-right symmetric video must give symmetric masks)."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, step as pstep
from tests import detectviews_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 8
FRAMES = (1, 17, 40)


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(29)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


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
    """One StepEngine(bs=2) and its detect engines, every pass computed once and shared."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    out = dict(eng=eng, vids=vids)
    for name, kw in (("tile_flip", dict(tile=True, flip=True)), ("tile", dict(tile=True))):
        rec = []
        de = eng.detect_engine(bs=BS, capacity=64, on_batch=lambda m, lg, sc: rec.append((m, lg.cpu().numpy(), sc.cpu().numpy())), **kw)
        first = _run(de, vids)
        counted = (de.n_videos, de.n_clips)
        de.on_batch = None
        out[name] = dict(de=de, rec=rec, first=first, counted=counted, again=_run(de, vids), packed=_run(de, vids, pack=True))
    return out


@pytest.mark.parametrize("name,tile,flip", [("tile_flip", True, True), ("tile", True, False)])
def test_detections_equal_a_numpy_restatement_of_the_engines_own_logits(world, name, tile, flip):
    w = world[name]
    views = detect.make_views(FHW[0], FHW[1], HW, tile, flip)
    V = len(views)
    assert V == (8 if flip else 4) and views[:2] == ([(0, 0, 0), (0, 0, 1)] if flip else [(0, 0, 0), (0, 24, 0)]) and views[-1][:2] == (8, 24)
    assert w["counted"] == (len(FRAMES), 1 + 3 + 6)
    it = iter(w["rec"])
    per = BS // V                                                      # clips of a batch
    npos = ntot = 0
    for frames, det in zip(world["vids"], w["first"]):
        F, H, W = frames.shape[:3]
        starts = evalstep.clip_starts(F, np.ones(F))
        merge, rows = ref.Merge(F, H, W, HW), []
        for i in range(0, len(starts), per):
            n = min(per, len(starts) - i)
            m, lg, sc = next(it)
            assert m == n * V and lg.shape == (m, 1, 8, HW, HW) and sc.shape == (m, 24)
            merge.add(lg[:, 0].reshape(V, n, 8, HW, HW), views, starts[i:i + n])
            rows += [sc[v * n + c] for c in range(n) for v in range(V)]                    # ring order: row0 + clip * V + view
        exp, merged = merge.masks(), merge.merged()
        assert (merge.num >= 1).all() and merge.num.max() == (8 if flip else 4)            # tiled: every pixel covered, the middle by all
        masks = det.masks.cpu().numpy()
        assert masks.shape == (F, H, W) and masks.dtype == np.uint8 and np.array_equal(masks, exp)
        assert det.views == views and det.counts.shape == (F,) and det.boxes.shape == (F, 4) and det.frame_scores.shape == (F,)
        for f in range(F):
            cnt = int(exp[f].sum())
            assert det.counts[f] == cnt and tuple(det.boxes[f]) == ref.box_of(exp[f]), (F, f)
            if cnt == 0:
                assert det.frame_scores[f] == 0.0
                continue
            r64, r32 = ref.score_refs(merged[f], exp[f])
            assert abs(float(det.frame_scores[f]) - r64) <= max(1e-6, 2.0 * abs(r32 - r64)), (F, f, det.frame_scores[f], r64, r32)
        npos += int(exp.sum()); ntot += exp.size
        scores = np.stack(rows)
        assert scores.shape == (len(starts) * V, 24)
        mean = scores[0].copy()
        for r in scores[1:]:
            mean = (mean + r).astype(np.float32)
        mean = (mean / np.float32(scores.shape[0])).astype(np.float32)
        assert det.label == evalstep.vote(scores) and np.array_equal(det.class_scores.view(np.int32), mean.view(np.int32))
        assert np.float32(det.class_score) == mean[det.label]
    assert next(it, None) is None
    print("detect engine, %s: %d of %d frame pixels positive" % (name, npos, ntot))
    assert 0 < npos < ntot                                             # the masks are neither empty nor full: the comparison means something


def test_the_views_of_one_clip_differ_and_the_ring_rows_follow_the_clips(world):
    """The flipped view of a random video is not its twin (the merge has something to average), and every frame's record names the ring row
    of its clip's first view."""
    w = world["tile_flip"]
    m, lg, _sc = w["rec"][0]
    assert m == 8 and not np.array_equal(lg[0], lg[1]) and not np.array_equal(lg[0], lg[2])
    de = w["de"]
    de.begin()
    de.add_video(world["vids"][1])
    de.results()
    rec = de.videos[0]
    rows = rec.pin.numpy()[:rec.F * 8].reshape(rec.F, 8)[:, 6]
    starts = evalstep.clip_starts(17, np.ones(17))
    for c, _k, f in ref.real_frames(starts, 17):
        assert rows[f] == rec.row0 + c * 8


@pytest.mark.parametrize("name", ["tile_flip", "tile"])
def test_batching_and_a_second_pass_give_equal_detections(world, name):
    w = world[name]
    assert len(w["first"]) == len(FRAMES) and [d.counts.size for d in w["first"]] == list(FRAMES)
    for other in ("again", "packed"):
        assert [_differs(a, b) for a, b in zip(w["first"], w[other])] == [[]] * len(FRAMES), (name, other)


def test_refused_videos_raise_and_change_nothing(world):
    eng, vids = world["eng"], world["vids"]
    small = eng.detect_engine(bs=4, capacity=64, tile=True, flip=True)                    # V = 8 views do not fit a batch of 4
    small.begin()
    state = lambda de: (de.pos, de.n_videos, de.n_clips, len(de.videos), len(de.batch), de.fill, len(de.live))
    before = state(small)
    with pytest.raises(ValueError, match="views"):
        small.add_video(vids[0])
    assert state(small) == before == (0, 0, 0, 0, 0, 0, 0)
    ring = eng.detect_engine(bs=BS, capacity=48, tile=True, flip=True)                    # 6 clips x 8 views = 48 rows > capacity - bs = 40
    ring.begin()
    assert ring.add_video(vids[1]) == 0                                                   # 3 x 8 = 24 rows
    before = state(ring)
    with pytest.raises(ValueError, match="capacity"):
        ring.add_video(vids[2])
    assert state(ring) == before
    got = ring.results()
    assert len(got) == 1 and _differs(got[0], world["tile_flip"]["first"][1]) == []
    with pytest.raises(ValueError):
        eng.detect_engine(bs=BS, capacity=64, views=[(9, 0, 0)]).detect(vids[0])          # 9 + 112 > 120: outside the frame
    assert len(eng.detect_engine(bs=BS, capacity=64, views=[(8, 24, 1), (0, 0, 0)]).detect(vids[0]).views) == 2


def test_the_default_arguments_take_the_path_they_took(world):
    eng, vids = world["eng"], world["vids"]
    plain = eng.detect_engine(bs=3, capacity=64)
    named = eng.detect_engine(bs=3, capacity=64, tile=False, flip=False, views=None)
    assert not plain.multi and not named.multi and named.ws_views is None
    a, b = _run(plain, vids), _run(named, vids)
    assert [_differs(x, y) for x, y in zip(a, b)] == [[]] * len(vids)
    h0, w0 = evalstep.centre_crop(FHW[0], FHW[1], HW)
    assert all(d.views == [(h0, w0, 0)] for d in a) and named.ws_views is None
    for d in a:                                                        # the centre crop: nothing outside it
        m = d.masks.cpu().numpy()
        assert not m[:, :h0].any() and not m[:, h0 + HW:].any() and not m[:, :, :w0].any() and not m[:, :, w0 + HW:].any()


def test_a_symmetric_video_gives_symmetric_masks_with_flip(world):
    """Every frame left-right symmetric: the flipped view's clip is the unflipped one, so the merged logit at x is (l[x] + l[S - 1 - x]) / 2,
    the same number at the mirrored pixel.  An un-flip in the wrong direction (or none) leaves l[x]: not symmetric."""
    eng = world["eng"]
    half = np.random.default_rng(31).integers(0, 256, (17, FHW[0], FHW[1] // 2, 3), dtype=np.uint8)
    video = np.concatenate([half, half[:, :, ::-1]], axis=2)
    assert video.shape == (17,) + FHW + (3,) and np.array_equal(video, video[:, :, ::-1])
    flip = eng.detect_engine(bs=BS, capacity=64, flip=True).detect(video)
    h0, w0 = evalstep.centre_crop(FHW[0], FHW[1], HW)
    assert flip.views == [(h0, w0, 0), (h0, w0, 1)]
    m = flip.masks.cpu().numpy()
    assert np.array_equal(m, m[:, :, ::-1]) and 0 < int(m.sum()) < 17 * HW * HW
    plain = eng.detect_engine(bs=BS, capacity=64).detect(video).masks.cpu().numpy()
    assert not np.array_equal(plain, plain[:, :, ::-1])               # the network itself is not mirror-symmetric: the test above can fail
