"""GPU: detect.DetectEngine(instances=K) at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as tests/test_detect_gpu.py is
sized (the tile + flip engine takes bs = 8: its 8 views of a clip share a batch).  The instance fields are checked against the numpy
restatement of tests/instances_ref.py applied to the engine's OWN masks, across the ways of batching and the ways of seeing a video; an engine
with instances=0 is today's engine in every field, and a pass between two train steps leaves the second step bit for bit what it is."""
import numpy as np
import pytest
import torch

from picons_amd import detect, ops, step as pstep, synthetic

from tests import instances_ref as ref

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


def _plain_differs(a, b):
    eq = dict(label=a.label == b.label, class_score=np.array_equal(_bits(a.class_score), _bits(b.class_score)),
              class_scores=np.array_equal(_bits(a.class_scores), _bits(b.class_scores)), counts=np.array_equal(a.counts, b.counts),
              boxes=np.array_equal(a.boxes, b.boxes), frame_scores=np.array_equal(_bits(a.frame_scores), _bits(b.frame_scores)),
              masks=torch.equal(a.masks, b.masks), views=a.views == b.views)
    return [k for k, v in eq.items() if not v]


def _inst_differs(a, b):
    names = ("inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")
    out = [k for k in names if not np.array_equal(getattr(a, k), getattr(b, k))]
    return out + ([] if (a.imap is None and b.imap is None) or torch.equal(a.imap, b.imap) else ["imap"])


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass computed once and shared.  Only the last test of the file trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    kw = dict(instances=K, min_area=MIN_AREA, instance_maps=True)
    de = eng.detect_engine(bs=BS, capacity=64, **kw)
    out = dict(eng=eng, vids=vids, de=de, first=_run(de, vids), again=_run(de, vids), packed=_run(de, vids, pack=True))
    out["conn4"] = _run(eng.detect_engine(bs=BS, capacity=64, instances=2, conn=4), vids)
    out["tile_flip"] = _run(eng.detect_engine(bs=8, capacity=128, tile=True, flip=True, **kw), vids)
    out["plain"] = _run(eng.detect_engine(bs=BS, capacity=64), vids)
    out["zero"] = _run(eng.detect_engine(bs=BS, capacity=64, instances=0, min_area=5, conn=4, instance_maps=True), vids)
    return out


def _against_restatement(dets, k, min_area, conn, maps):
    """Every instance field of `dets` against the restatement of their own masks -> (frames, frames with an instance, overflow frames)."""
    seen = some = over = 0
    for F, d in zip(FRAMES, dets):
        masks = d.masks.cpu().numpy()
        assert masks.shape == (F,) + FHW
        rec, imap, runs = ref.video_instances(masks, conn, min_area, k)
        n, kept, _runs, flags, areas, boxes, first = ops.decode_instances(rec, k)
        assert np.array_equal(flags & 1, runs > ops.INST_MAX_RUNS)
        for f in np.flatnonzero(flags & 1):                         # the engine's substitute: one instance, the frame's own count and box
            assert d.counts[f] > ops.INST_MAX_RUNS >= min_area
            n[f] = kept[f] = 1
            areas[f, 0], boxes[f, 0], first[f, 0] = d.counts[f], d.boxes[f], -1
        for name, want in (("inst_n", n), ("inst_kept", kept), ("inst_flags", flags), ("inst_areas", areas), ("inst_boxes", boxes), ("inst_first", first)):
            got = getattr(d, name)
            assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (name, F)
        assert d.inst_areas.shape == (F, k) and d.inst_boxes.shape == (F, k, 4)
        if maps:
            assert d.imap.dtype == torch.uint8 and torch.equal(d.imap.cpu(), torch.from_numpy(imap))
            others = (imap == 255).reshape(F, -1).sum(1)
        else:
            assert d.imap is None
            others = np.array([np.count_nonzero(imap[f] == 255) for f in range(F)])
        ok = (flags & 1) == 0
        assert np.array_equal((d.inst_areas.sum(1) + others)[ok], d.counts[ok])       # kept instances and the other foreground: every positive pixel
        for f in np.flatnonzero(d.inst_kept > 0):
            x0, y0, x1, y1 = d.inst_boxes[f, 0]
            X0, Y0, X1, Y1 = d.boxes[f]
            assert X0 <= x0 < x1 <= X1 and Y0 <= y0 < y1 <= Y1, (F, f)                  # the top-1 box lies within the frame's box
        seen += F; some += int((ok & (d.inst_kept > 0)).sum()); over += int((~ok).sum())
    return seen, some, over


def test_instances_equal_the_restatement_of_the_engines_own_masks(world):
    seen, some, over = _against_restatement(world["first"], K, MIN_AREA, 8, True)
    print("instances: %d frames, %d labelled with an instance, %d over the run cap" % (seen, some, over))
    assert seen == sum(FRAMES) and some > 0                          # the comparison means something: frames were labelled, not all fell back
    _against_restatement(world["conn4"], 2, 1, 4, False)
    for d in world["first"]:
        tubes = d.instance_tubes()
        assert sum(int(np.count_nonzero(a)) for _t0, _t1, _b, a, _s in tubes) == int(d.inst_kept.sum())      # every instance in exactly one tube


def test_batching_a_second_pass_and_the_views_agree_with_the_restatement(world):
    first = world["first"]
    for name in ("again", "packed"):
        assert [_plain_differs(a, b) + _inst_differs(a, b) for a, b in zip(first, world[name])] == [[]] * len(first), name
    assert _against_restatement(world["packed"], K, MIN_AREA, 8, True)[0] == sum(FRAMES)
    tf = world["tile_flip"]
    assert all(len(d.views) == 8 for d in tf)
    assert _against_restatement(tf, K, MIN_AREA, 8, True)[0] == sum(FRAMES)


def test_instances_0_is_the_engine_without_the_arguments(world):
    eng, plain, zero, first = world["eng"], world["plain"], world["zero"], world["first"]
    assert [_plain_differs(a, b) for a, b in zip(plain, zero)] == [[]] * len(plain)
    assert [_plain_differs(a, b) for a, b in zip(plain, first)] == [[]] * len(plain)          # nor do the instances change an existing field
    for d in plain + zero:
        assert d.inst_n is d.inst_kept is d.inst_flags is d.inst_areas is d.inst_boxes is d.inst_first is d.imap is None
        with pytest.raises(ValueError):
            d.instance_tubes()
    a, b = eng.detect_engine(bs=BS, capacity=64), eng.detect_engine(bs=BS, capacity=64, instances=0)
    for de in (a, b, world["de"]):
        de.begin()
        de.add_video(world["vids"][1])
    F, C = FRAMES[1], a.C
    assert a.videos[0].dev.numel() == b.videos[0].dev.numel() == F * 8 + C + 2 and b.videos[0].imap is None
    assert world["de"].videos[0].dev.numel() == F * 8 + C + 2 + F * (4 + 6 * K)                # behind the class vector: nothing before it moves
    for de in (a, b, world["de"]):
        de.results()


def test_constructor_refusals(world):
    eng = world["eng"]
    with pytest.raises(ValueError, match="masks=True"):
        eng.detect_engine(bs=BS, capacity=64, instances=4, masks=False)
    for kw in (dict(instances=33), dict(instances=-1), dict(instances=4, conn=5), dict(instances=4, min_area=0)):
        with pytest.raises(ValueError, match="instances"):
            eng.detect_engine(bs=BS, capacity=64, **kw)
    assert eng.detect_engine(bs=BS, capacity=64, masks=False).detect(world["vids"][0]).masks is None         # without instances still allowed


def test_an_instance_pass_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with instances on the step engine's weights, train step, against the same two steps on a fresh engine: the
    second step's losses, the gradient of conv1.Mixed_4f.b1b.conv3d.weight, the running statistics and the step count are equal bit for bit."""
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
            assert all(d.inst_kept is not None and d.imap is not None for d in dets)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
