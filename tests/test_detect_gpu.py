"""GPU: detect.DetectEngine (unlabelled uint8 video in; per-frame masks, boxes, scores and the video's class out) at hw = 112 with frames of
120 x 136, so that both crop offsets are non-zero, bs = 3 and synthetic weights, as tests/test_evalstep_gpu.py is sized.  The detections are
checked against a torch restatement fed the engine's own logits (which are checked against CapsNet.eval() on the same weights), against the
counts evalstep.EvalEngine leaves for the same video, across the ways of batching, after a refused video, and a detection pass between two
train steps must leave the second step bit for bit what it is."""
import numpy as np
import pytest
import torch

from picons_amd import detect, evalstep, model as pmodel, step as pstep, synthetic

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40, 33)


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    rng = np.random.default_rng(23)
    return [rng.integers(0, 256, (F,) + FHW + (3,), dtype=np.uint8) for F in FRAMES]


def _run(de, vids, pack=False):
    de.begin(pack)
    assert [de.add_video(v) for v in vids] == list(range(len(vids)))
    return de.results()


def _differs(a, b, masks=True):
    """The fields in which two detections differ (bit for bit), as a list of names: empty if they are the same."""
    bits = lambda x: np.asarray(x, np.float32).view(np.int32)
    eq = dict(label=a.label == b.label, class_score=np.array_equal(bits(a.class_score), bits(b.class_score)),
              class_scores=np.array_equal(bits(a.class_scores), bits(b.class_scores)), counts=np.array_equal(a.counts, b.counts),
              boxes=np.array_equal(a.boxes, b.boxes), frame_scores=np.array_equal(bits(a.frame_scores), bits(b.frame_scores)))
    if masks:
        eq["masks"] = torch.equal(a.masks, b.masks)
    return [k for k, v in eq.items() if not v]


def _same(a, b, masks=True):
    return not _differs(a, b, masks)


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) with its detect_engine(3): one recorded pass over the videos, the same pass again, packed, without masks, and on a
    ring small enough to wrap -- computed once and shared.  Only the last test of the file trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    state = eng.state_dict()
    rec = []
    de = eng.detect_engine(bs=BS, capacity=64, on_batch=lambda m, lg, sc: rec.append((m, lg.cpu().numpy(), sc.cpu().numpy())))
    vids = _videos()
    first = _run(de, vids)
    counted = (de.n_videos, de.n_clips)
    de.on_batch = None
    again = _run(de, vids)
    packed = _run(de, vids, pack=True)
    bare = eng.detect_engine(bs=BS, capacity=64, masks=False)
    no_masks = _run(bare, vids)
    small = eng.detect_engine(bs=BS, capacity=8)
    ring = [vids[0], vids[1], vids[3], vids[1]]                        # 1 + 3 + 5 + 3 clip rows through a ring of 8
    wrapped = _run(small, ring)
    wrapped_packed = _run(small, ring, pack=True)
    return dict(eng=eng, de=de, small=small, vids=vids, rec=rec, first=first, again=again, packed=packed, no_masks=no_masks, wrapped=wrapped,
                wrapped_packed=wrapped_packed, state=state, counted=counted)


def _clips(frames):
    """The clips of an unlabelled video as the reference's loop cuts them: [n][8][HW][HW][3] float32 = frame / 255., zeros past the end."""
    F = frames.shape[0]
    h0, w0 = evalstep.centre_crop(frames.shape[1], frames.shape[2], HW)
    assert h0 > 0 and w0 > 0
    starts = evalstep.clip_starts(F, np.ones(F))
    crop = frames[:, h0:h0 + HW, w0:w0 + HW] / 255.
    out = np.zeros((len(starts), 8, HW, HW, 3), np.float32)
    for c, s in enumerate(starts):
        for k in range(8):
            if s + 2 * k < F:
                out[c, k] = crop[s + 2 * k]
    return starts, out, (h0, w0)


def test_detections_equal_a_torch_restatement_of_the_engines_logits(world):
    net = pmodel.CapsNet(pt_path=None, hw=HW, init="conditioned").cuda()
    net.load_state_dict(world["state"])
    net.eval(); net.training = False
    it = iter(world["rec"])
    assert world["counted"] == (len(FRAMES), 1 + 3 + 6 + 5)
    npos = ntot = 0
    for frames, det in zip(world["vids"], world["first"]):
        F, H, W = frames.shape[:3]
        starts, clips, (h0, w0) = _clips(frames)
        logits, scores = [], []
        for i in range(0, len(starts), BS):
            m, s_, p_ = next(it)
            assert m == min(BS, len(starts) - i) and s_.shape == (m, 1, 8, HW, HW) and p_.shape == (m, 24)
            data = torch.from_numpy(np.transpose(clips[i:i + BS], [0, 4, 1, 2, 3])).float().cuda()
            empty = torch.full((m, 1), 500, dtype=torch.int64, device="cuda")
            with torch.no_grad():
                o, p, _ = net(data, empty, empty, 0, 0)
            d_o, d_p = float(np.abs(o.cpu().numpy() - s_).max()), float(np.abs(p.cpu().numpy() - p_).max())
            print("detect engine vs CapsNet.eval: F=%d batch of %d  |dlogits| %.2e |dscores| %.2e" % (F, m, d_o, d_p))
            assert d_o <= 1e-3 and d_p <= 1e-3
            logits.append(s_); scores.append(p_)
        logits, scores = np.concatenate(logits)[:, 0], np.concatenate(scores)
        pos = (torch.sigmoid(torch.from_numpy(logits)) >= 0.5).numpy()
        exp = np.zeros((F, H, W), np.uint8)
        for c, s in enumerate(starts):                                 # the clip interleave undone by hand, pasted into full frames
            for k in range(8):
                if s + 2 * k < F:
                    exp[s + 2 * k, h0:h0 + HW, w0:w0 + HW] = pos[c, k]
        masks = det.masks.cpu().numpy()
        assert masks.shape == (F, H, W) and masks.dtype == np.uint8 and np.array_equal(masks, exp)
        assert det.counts.shape == (F,) and det.boxes.shape == (F, 4) and det.frame_scores.shape == (F,)
        for f in range(F):
            ys, xs = np.nonzero(exp[f])
            box = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if ys.size else (0, 0, 0, 0)
            assert det.counts[f] == ys.size and tuple(det.boxes[f]) == box, (F, f)
            assert (0.5 <= det.frame_scores[f] <= 1.0) if ys.size else det.frame_scores[f] == 0.0
        npos += int(exp.sum()); ntot += F * HW * HW
        mean = scores[0].copy()
        for r in scores[1:]:
            mean = (mean + r).astype(np.float32)
        mean = (mean / np.float32(scores.shape[0])).astype(np.float32)
        assert det.label == evalstep.vote(scores) and np.array_equal(det.class_scores.view(np.int32), mean.view(np.int32))
        assert np.float32(det.class_score) == mean[det.label]
        tubes = det.tubes()
        assert all(det.counts[t0:t1 + 1].all() for t0, t1, _b, _s in tubes) and sum(t1 - t0 + 1 for t0, t1, _b, _s in tubes) == int((det.counts > 0).sum())
    assert next(it, None) is None
    print("detect engine: %d of %d crop pixels positive" % (npos, ntot))
    assert 0 < npos < ntot                                             # the masks are neither empty nor full: the comparison means something


def test_masks_agree_with_the_counts_the_evaluator_leaves(world):
    """A video whose truth is non-zero in every frame, so that EvalEngine keeps every clip: per frame, the intersection and union of the
    DetectEngine's mask with the cropped truth, in numpy, are the rows EvalEngine leaves in `counts`."""
    frames = world["vids"][3]
    F, H, W = frames.shape[:3]
    truth = np.zeros((F, H, W), np.uint8)
    truth[:, 30:70, 40:90] = 1
    truth[::2, 10:110, 20:40] = 1
    ee = world["eng"].eval_engine(bs=BS, capacity=64)
    ee.begin()
    assert ee.add_video(frames, truth, 2) == 5
    ee.results()
    rows = ee.counts[:5 * 8].cpu().numpy().reshape(5, 8, 3)
    masks = world["first"][3].masks.cpu().numpy()
    h0, w0 = evalstep.centre_crop(H, W, HW)
    starts = evalstep.clip_starts(F, np.ones(F))
    seen = 0
    for c, s in enumerate(starts):
        for k in range(8):
            f = s + 2 * k
            if f >= F:
                continue
            m, t = masks[f, h0:h0 + HW, w0:w0 + HW] != 0, truth[f, h0:h0 + HW, w0:w0 + HW] != 0
            assert tuple(rows[c, k]) == (int((m & t).sum()), int((m | t).sum()), int(t.sum())), (c, k, f)
            assert not masks[f, :h0].any() and not masks[f, h0 + HW:].any() and not masks[f, :, :w0].any() and not masks[f, :, w0 + HW:].any()
            seen += 1
    assert seen == F


def test_batching_ring_wrap_no_masks_and_a_second_pass_give_equal_detections(world):
    first = world["first"]
    assert len(first) == len(FRAMES) and [d.counts.size for d in first] == list(FRAMES)
    for name in ("again", "packed"):
        assert [_differs(a, b) for a, b in zip(first, world[name])] == [[]] * len(first), name
    assert all(d.masks is None for d in world["no_masks"]) and all(_same(a, b, masks=False) for a, b in zip(first, world["no_masks"]))
    ring = [first[0], first[1], first[3], first[1]]                    # 12 clip rows through a ring of 8: the third video starts at row 0 again
    for name in ("wrapped", "wrapped_packed"):
        assert [_differs(a, b) for a, b in zip(ring, world[name])] == [[]] * 4, name
    assert world["small"].n_clips == 12 > world["small"].capacity
    de = world["de"]
    one = de.detect(world["vids"][1])
    assert _same(one, first[1])
    out, pred = de.outputs()                                           # the last batch: the one video's three clips
    assert out.shape == (3, 1, 8, HW, HW) and pred.shape == (3, 24)


def test_a_refused_video_raises_and_changes_nothing(world):
    de, small, vids = world["de"], world["small"], world["vids"]
    de.begin()
    de.add_video(vids[1])
    state = (de.pos, de.n_videos, de.n_clips, len(de.videos), len(de.batch), de.fill)
    f = vids[1]
    bad = [f.astype(np.float32), f[0], f[..., :2], f[:0], f[:, :HW - 1], f[:, :, :HW - 2], torch.from_numpy(f).short(), "video.avi", None]
    for v in bad:
        with pytest.raises(ValueError):
            de.add_video(v)
        assert (de.pos, de.n_videos, de.n_clips, len(de.videos), len(de.batch), de.fill) == state
    assert de.add_video(torch.from_numpy(vids[0])) == 1                # a host tensor and a device tensor are taken as numpy is
    assert de.add_video(torch.from_numpy(vids[0]).cuda()) == 2
    res = de.results()
    fresh = detect.DetectEngine(bs=BS, hw=HW, state=world["state"], capacity=64)
    want = fresh.detect(vids[0])
    assert len(res) == 3 and _same(res[1], want) and _same(res[2], want) and _same(res[0], world["first"][1])
    # one video that needs more than capacity - bs rows of the ring
    small.begin()
    with pytest.raises(ValueError, match="capacity"):
        small.add_video(vids[2])
    assert small.pos == 0 and small.n_videos == 0 and small.videos == []
    with pytest.raises(ValueError, match="multiple of 4"):
        detect.DetectEngine(bs=BS, hw=110, state=world["state"])


def test_a_detection_pass_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass on the step engine's weights, train step against the same two steps on a fresh engine: the second step's
    losses and the gradient of conv1.Mixed_4f.b1b.conv3d.weight are equal bit for bit, and so are the running statistics and the step count."""
    eng, de = world["eng"], world["de"]
    ref = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, detect_between in ((eng, True), (ref, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if detect_between:
            trained = _run(de, world["vids"][:2])
            after_first = e.state_dict()                  # (read after the pass: results() has waited for the stream the pass ran on)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
    # the pass saw the step engine's weights as the first train step left them (it waited for the step's lanes, not the host for the step):
    # an engine of its own holding that state gives the same detections
    own = detect.DetectEngine(bs=BS, hw=HW, state=after_first, capacity=64)
    assert all(_same(a, b) for a, b in zip(_run(own, world["vids"][:2]), trained))
