"""GPU: detect.DetectEngine.mask_runs at hw = 112 with frames of 120 x 136, bs = 3 and synthetic weights, as tests/test_instances_gpu.py is
sized (the tile + flip engine takes bs = 8).  The runs of a pass decode to the engine's OWN masks and maps of ranks, byte for byte; they are
the words of the numpy restatement (tests/mask_runs_ref.py); across the ways of batching, a second pass and a second call they are equal; the
call changes no field of a detection and no buffer size; a pass plus export between two train steps changes nothing."""
import numpy as np
import pytest
import torch

from picons_amd import detect, ops, step as pstep, synthetic

from tests import mask_runs_ref as ref

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
FRAMES = (1, 17, 40)
K, MIN_AREA = 8, 3
FIELDS = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")


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


def _differs(a, b):
    out = [k for k in FIELDS if not np.array_equal(getattr(a, k), getattr(b, k))]
    out += [k for k in ("class_score", "class_scores", "frame_scores") if not np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k)))]
    out += [k for k in ("masks", "imap") if not torch.equal(getattr(a, k), getattr(b, k))]
    if a.label != b.label or a.views != b.views:
        out.append("label/views")
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.offsets, b.offsets) and np.array_equal(a.runs, b.runs)


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) and its detect engines, every pass and export computed once and shared.  Only the last test trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    vids = _videos()
    kw = dict(instances=K, min_area=MIN_AREA, instance_maps=True)
    de = eng.detect_engine(bs=BS, capacity=64, **kw)
    out = dict(eng=eng, vids=vids, de=de)
    out["first"] = _run(de, vids)
    out["dense"] = [(d.masks.cpu().numpy(), d.imap.cpu().numpy()) for d in out["first"]]
    out["words"] = [r.dev.numel() for r in de.videos]
    out["runs"] = (de.mask_runs("masks"), de.mask_runs("imap"))
    out["second_call"] = (de.mask_runs("masks"), de.mask_runs("imap"))
    out["subset"] = de.mask_runs("imap", videos=[1])
    out["after"] = de.results()                                      # the detections once more, behind the exports
    _run(de, vids)
    out["second_pass"] = (de.mask_runs("masks"), de.mask_runs("imap"))
    _run(de, vids, pack=True)
    out["packed"] = (de.mask_runs("masks"), de.mask_runs("imap"))
    never = eng.detect_engine(bs=BS, capacity=64, **kw)               # an engine on which the method is never called
    out["never"] = _run(never, vids)
    out["never_words"] = [r.dev.numel() for r in never.videos]
    tf = eng.detect_engine(bs=8, capacity=128, tile=True, flip=True, **kw)
    out["tf"] = _run(tf, vids)
    out["tf_runs"] = (tf.mask_runs("masks"), tf.mask_runs("imap"))
    return out


def test_runs_decode_to_the_engines_own_masks_and_maps(world):
    masks, imaps = world["runs"]
    assert len(masks) == len(imaps) == len(FRAMES)
    n_runs = 0
    for F, d, (dm, di), rm, ri in zip(FRAMES, world["first"], world["dense"], masks, imaps):
        assert isinstance(rm, detect.MaskRuns) and rm.shape == ri.shape == (F,) + FHW
        assert rm.runs.dtype == np.uint32 and rm.offsets.dtype == np.int64 and rm.offsets.shape == (F + 1,)
        assert np.array_equal(rm.dense(), dm) and np.array_equal(ri.dense(), di)
        assert set(np.unique(dm).tolist()) <= {0, 1} and set(np.unique(rm.runs[:, 0] >> 24).tolist()) <= {1}
        assert np.array_equal(rm.areas(), d.counts.astype(np.int64)) and np.array_equal(ri.areas(), d.counts.astype(np.int64))
        for f in (0, F // 2, F - 1):
            assert np.array_equal(rm.dense(f), dm[f]) and np.array_equal(ri.dense(f), di[f])
            y, x0, x1, v = ri.frame(f)
            assert ((0 <= y) & (y < FHW[0]) & (x0 < x1) & (x1 <= FHW[1]) & (v > 0)).all() and int((x1 - x0).sum()) == int(d.counts[f])
        # the very words of the restatement, and of the host encoder
        for got, dense in ((rm, dm), (ri, di)):
            index, runs = ref.runs_of(dense)
            assert np.array_equal(got.runs, runs) and np.array_equal(got.offsets, index[::FHW[0]].astype(np.int64))
            assert _same(got, detect.MaskRuns.from_dense(dense))
            assert got.nbytes == runs.nbytes + 8 * (F + 1)
        n_runs += rm.runs.shape[0]
    assert n_runs > 0                                                # the synthetic weights do give foreground
    assert any(len(set(np.unique(ri.runs[:, 0] >> 24).tolist())) > 1 for ri in imaps)      # more than one rank value went through


def test_a_second_call_a_second_pass_and_packing_give_equal_runs(world):
    for name in ("second_call", "second_pass", "packed"):
        for a_list, b_list in zip(world["runs"], world[name]):
            assert [_same(a, b) for a, b in zip(a_list, b_list)] == [True] * len(FRAMES), name
    assert world["runs"][0][0].runs is not world["second_call"][0][0].runs      # arrays of their own, not views of the staging


def test_videos_selects_a_subset(world):
    sub = world["subset"]
    assert len(sub) == 1 and _same(sub[0], world["runs"][1][1])
    de = world["de"]
    got = de.mask_runs("masks", videos=[2, 0, 2])
    assert [_same(g, world["packed"][0][i]) for g, i in zip(got, (2, 0, 2))] == [True] * 3
    assert de.mask_runs("masks", videos=[]) == []


def test_tile_and_flip(world):
    masks, imaps = world["tf_runs"]
    for d, rm, ri in zip(world["tf"], masks, imaps):
        assert len(d.views) == 8
        assert np.array_equal(rm.dense(), d.masks.cpu().numpy()) and np.array_equal(ri.dense(), d.imap.cpu().numpy())
        assert np.array_equal(rm.areas(), d.counts.astype(np.int64))


def test_the_call_changes_no_field_and_no_buffer(world):
    assert world["words"] == world["never_words"]
    for a, b, c in zip(world["first"], world["after"], world["never"]):
        assert _differs(a, b) == [] and _differs(a, c) == []
    for d, (dm, di) in zip(world["after"], world["dense"]):          # the device maps themselves are as they were
        assert np.array_equal(d.masks.cpu().numpy(), dm) and np.array_equal(d.imap.cpu().numpy(), di)


def test_a_video_exported_in_several_ranges(world, monkeypatch):
    """The limits of one pc_mask_run_index call lowered so that the 17- and the 40-frame video take several ranges: equal runs."""
    de = world["de"]
    monkeypatch.setattr(detect, "RUN_RANGE_PIXELS", 7 * FHW[0] * FHW[1] + 5)
    assert detect.run_ranges(40, *FHW) == [(0, 7), (7, 7), (14, 7), (21, 7), (28, 7), (35, 5)]
    got = de.mask_runs("imap")
    monkeypatch.setattr(detect, "RUN_RANGE_ROWS", 3 * FHW[0] + 1)
    assert detect.run_ranges(17, *FHW) == [(0, 3), (3, 3), (6, 3), (9, 3), (12, 3), (15, 2)]
    got3 = de.mask_runs("imap", videos=[1, 2])
    assert [_same(a, b) for a, b in zip(got, world["packed"][1])] == [True] * 3
    assert [_same(a, b) for a, b in zip(got3, world["packed"][1][1:])] == [True] * 2


def test_refusals_are_value_errors_before_anything_is_enqueued(world):
    eng, de, vids = world["eng"], world["de"], world["vids"]
    for bad in ("mask", "probs", None, 0):
        with pytest.raises(ValueError, match="which"):
            de.mask_runs(bad)
    for bad in ([3], [-1], [0, 5]):
        with pytest.raises(ValueError, match="video"):
            de.mask_runs("masks", videos=bad)
    records = eng.detect_engine(bs=BS, capacity=64, masks=False)
    _run(records, vids[:1])
    with pytest.raises(ValueError, match="masks=False"):
        records.mask_runs()
    for kw in (dict(), dict(instances=K), dict(instances=K, instance_links=1)):      # no map of ranks kept for the caller
        plain = eng.detect_engine(bs=BS, capacity=64, **kw)
        with pytest.raises(ValueError, match="no finished pass"):
            plain.mask_runs()
        d = _run(plain, vids[:1])[0]
        with pytest.raises(ValueError, match="instance_maps"):
            plain.mask_runs("imap")
        assert np.array_equal(plain.mask_runs()[0].dense(), d.masks.cpu().numpy())
        plain.begin()
        with pytest.raises(ValueError, match="no finished pass"):
            plain.mask_runs()
    packed = eng.detect_engine(bs=BS, capacity=64)
    packed.begin(True)
    packed.add_video(vids[0])                                        # one clip waits for a full batch: the pass is not finished
    with pytest.raises(ValueError, match="no finished pass"):
        packed.mask_runs()
    d = packed.results()[0]
    assert np.array_equal(packed.mask_runs()[0].dense(), d.masks.cpu().numpy())


def test_a_pass_and_export_between_two_train_steps_changes_nothing(world):
    """Train step, detection pass with both exports on the step engine's weights, train step, against the same two steps on a fresh engine:
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
            for which in ("masks", "imap"):
                for d, r in zip(dets, de.mask_runs(which)):
                    assert np.array_equal(r.dense(), getattr(d, which).cpu().numpy())
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
