"""GPU: evalstep.EvalEngine (the f-mAP / v-mAP evaluation from decoded uint8 video) at hw = 112 with frames of 120 x 136, so that both crop
offsets are non-zero.  The accumulation is checked apart from the network (teacher-forced: the oracle's MapState fed the engine's own logits),
the network against CapsNet.eval() holding the same weights, the ways of batching against each other, the drop-in's PICONS_EVAL_ENGINE=1
against the engine called directly, and an evaluation pass between two train steps must leave the second step bit for bit what it is."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import evalmetrics as oe
from picons_amd import evalstep, model as pmodel, step as pstep, synthetic

pytestmark = pytest.mark.gpu
HW, FHW, BS = 112, (120, 136), 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin")
TABLES = ("frame_ious", "video_ious", "n_tot_frames", "n_vids")


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _videos():
    """Four videos: three synthetic ones (video 1: the box lies outside the centre crop, the video is skipped) and one of 33 frames with truth
    in every frame -- five clips, a full batch and a ragged one, the last clip with one real frame -- whose truth takes the values 1, 2 and 255."""
    vids = synthetic.make_eval_videos_u8(3, seed=11, hw=HW, frames_hw=FHW)
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (33,) + FHW + (3,), dtype=np.uint8)
    truth = np.zeros((33,) + FHW + (1,), np.uint8)
    truth[:, 30:70, 40:90] = 1
    truth[::3, 50:60, 50:60] = 2
    truth[32, 20:25, 20:25] = 255
    return vids + [(frames, truth, 7)]


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in TABLES) and a["n_correct"] == b["n_correct"]


@pytest.fixture(scope="module")
def world():
    """One StepEngine(bs=2) with its eval_engine(3): one recorded pass over the videos, the same pass again, packed, on a ring small enough to
    wrap -- computed once and shared.  Only the last test of the file trains the engine."""
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    state = eng.state_dict()
    rec = []
    ee = eng.eval_engine(bs=BS, capacity=64, on_batch=lambda m, lg, sc: rec.append((m, lg.cpu().numpy(), sc.cpu().numpy())))
    vids = _videos()
    first = ee.evaluate(vids)
    counted = (ee.n_videos, ee.n_skipped, ee.n_clips)
    ee.on_batch = None
    again = ee.evaluate(vids)
    packed = ee.evaluate(vids, pack=True)
    small = eng.eval_engine(bs=BS, capacity=8)
    wrapped = small.evaluate(vids)
    wrapped_packed = small.evaluate(vids, pack=True)
    return dict(eng=eng, ee=ee, small=small, vids=vids, rec=rec, first=first, again=again, packed=packed, wrapped=wrapped,
                wrapped_packed=wrapped_packed, state=state, counted=counted)


def _oracle_clips(frames, truth, label):
    h0, w0 = evalstep.centre_crop(frames.shape[1], frames.shape[2], HW)
    assert h0 > 0 and w0 > 0
    return oe.make_clips(frames[:, h0:h0 + HW, w0:w0 + HW] / 255., truth[:, h0:h0 + HW, w0:w0 + HW], label)


def test_teacher_forced_tables_equal_the_oracles(world):
    st = oe.MapState(24)
    it = iter(world["rec"])
    seen = skipped = nclips = 0
    for frames, truth, label in world["vids"]:
        clips = _oracle_clips(frames, truth, label)
        if not clips:
            skipped += 1
            continue
        seen += 1; nclips += len(clips)
        segs, preds = [], []
        for i in range(0, len(clips), BS):
            m, s_, p_ = next(it)
            assert m == min(BS, len(clips) - i) and s_.shape == (m, 1, 8, HW, HW) and p_.shape == (m, 24)
            segs.append(s_); preds.append(p_)
        gt = np.stack([c[1] for c in clips]).reshape(-1, HW, HW, 1)
        st.add_video(np.concatenate(segs), gt, np.concatenate(preds), label)
    assert next(it, None) is None
    r = world["first"]
    assert (seen, skipped, nclips) == world["counted"] and skipped == 1
    assert np.array_equal(r["frame_ious"], st.frame_ious) and np.array_equal(r["video_ious"], st.video_ious)
    assert np.array_equal(r["n_tot_frames"], st.n_tot_frames) and np.array_equal(r["n_vids"], st.n_vids) and r["n_correct"] == st.n_correct
    assert r["n_tot_frames"].sum() > 0 and r["n_vids"].sum() == 3


def test_outputs_match_capsnet_eval_on_the_same_weights(world):
    net = pmodel.CapsNet(pt_path=None, hw=HW, init="conditioned").cuda()
    net.load_state_dict(world["state"])
    net.eval(); net.training = False
    it = iter(world["rec"])
    for frames, truth, label in world["vids"]:
        clips = _oracle_clips(frames, truth, label)
        for i in range(0, len(clips), BS):
            m, s_, p_ = next(it)
            data = torch.from_numpy(np.transpose(np.stack([c[0] for c in clips[i:i + BS]]), [0, 4, 1, 2, 3])).float().cuda()
            empty = torch.full((m, 1), 500, dtype=torch.int64, device="cuda")
            with torch.no_grad():
                o, p, _ = net(data, empty, empty, 0, 0)
            d_o, d_p = float(np.abs(o.cpu().numpy() - s_).max()), float(np.abs(p.cpu().numpy() - p_).max())
            print("eval engine vs CapsNet.eval: batch of %d  |dlogits| %.2e |dscores| %.2e" % (m, d_o, d_p))
            assert d_o <= 1e-3 and d_p <= 1e-3


def test_batching_ring_wrap_and_a_second_pass_give_equal_tables(world):
    first = world["first"]
    assert _same(first, world["again"])                    # a second pass after begin()
    assert _same(first, world["packed"])                   # clips of consecutive videos sharing batches
    assert _same(first, world["wrapped"])                  # 9 clip rows through a ring of 8: the last video starts at row 0 again
    assert _same(first, world["wrapped_packed"])
    assert world["counted"][2] > world["small"].capacity
    ee = world["ee"]
    ee.evaluate(world["vids"][:1], pack=True)
    out, pred = ee.outputs()                               # the last batch: the one video's clips, a short batch
    assert out.shape == (ee.m, 1, 8, HW, HW) and pred.shape == (ee.m, 24) and 1 <= ee.m <= BS


def test_a_skipped_videos_buffer_is_replaced_while_another_video_waits(world):
    """pack=True on a fresh engine: the first video's two clips wait for a full batch (its buffer is in use), the second is skipped (its small
    buffer is free at once), the third is larger than that buffer, which is dropped for a new one.  Same tables as the unpacked pass."""
    vids = world["vids"]
    skipped = (vids[1][0][:9], vids[1][1][:9], vids[1][2])
    seq = [vids[0], skipped, vids[3]]
    fresh = world["eng"].eval_engine(bs=BS, capacity=16)
    packed = fresh.evaluate(seq, pack=True)
    sizes = sorted(e["buf"].numel() for e in fresh.pool)
    assert fresh.n_skipped == 1 and len(sizes) == 2 and sizes[0] >= vids[0][0].nbytes and sizes[1] >= vids[3][0].nbytes and all(e["free"] is not None for e in fresh.pool)
    assert _same(packed, fresh.evaluate(seq, pack=False)) and packed["n_vids"].sum() == 2


def test_bad_videos_raise_and_change_nothing(world):
    ee, small = world["ee"], world["small"]
    frames, truth, label = world["vids"][0]
    F = frames.shape[0]
    ee.begin(pack=False)
    ee.add_video(frames, truth, label)
    state = (ee.pos, ee.n_videos, ee.n_clips, ee.tables.clone(), ee.counts.clone())
    bad = [(frames.astype(np.float32), truth, label), (frames, truth.astype(np.float32), label), (frames[0], truth, label), (frames[..., :2], truth, label),
           (frames[:, :HW - 1], truth[:, :HW - 1], label), (frames[:, :, :HW - 2], truth[:, :, :HW - 2], label), (frames, truth[:F - 1], label),
           (frames, truth[:, 1:], label), (frames, truth, 24), (frames, truth, -1), (frames, truth, 1.5), ("video.avi", truth, label)]
    for v, t, l in bad:
        with pytest.raises(ValueError):
            ee.add_video(v, t, l)
        assert (ee.pos, ee.n_videos, ee.n_clips) == state[:3]
    assert torch.equal(ee.tables, state[3]) and torch.equal(ee.counts, state[4])
    # one video that needs more than capacity - bs rows of the ring
    small.begin()
    long_truth = np.zeros((100,) + FHW, np.uint8); long_truth[:, 50:60, 60:70] = 1
    with pytest.raises(ValueError, match="capacity"):
        small.add_video(np.zeros((100,) + FHW + (3,), np.uint8), long_truth, 0)
    assert small.pos == 0 and small.n_videos == 0 and int(small.tables.abs().sum()) == 0
    # a host tensor and a device tensor are taken as numpy is
    ee.begin()
    ee.add_video(torch.from_numpy(frames), torch.from_numpy(truth), label)
    ee.add_video(torch.from_numpy(frames).cuda(), torch.from_numpy(truth[..., 0]).cuda(), label)
    r = ee.results()
    assert r["n_vids"].sum() == 2 and r["n_vids"][label, 0] == 2


def test_dropin_with_the_eval_engine_switch(world, tmp_path, monkeypatch, capsys):
    """dropin/evaluate_ucf101.py with PICONS_EVAL_ENGINE=1 on the synthetic uint8 videos: two checkpoints with the same weights, two printed
    lines, the tie pruned as without the switch, and the tables of the engine called directly."""
    monkeypatch.syspath_prepend(DROPIN)
    monkeypatch.setenv("PICONS_SYNTHETIC", "1"); monkeypatch.setenv("PICONS_EVAL_VIDEOS", "3"); monkeypatch.setenv("PICONS_EVAL_ENGINE", "1")
    monkeypatch.delenv("PICONS_EVAL_PACK", raising=False); monkeypatch.delenv("PICONS_DATASET", raising=False); monkeypatch.delenv("PICONS_KEEP_CKPTS", raising=False)
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in ("models", "utils") or k.startswith(("models.", "utils."))}
    try:
        for tag in ("a", "b"):
            torch.save(world["state"], str(tmp_path / ("best_model_train_%s.pth" % tag)))
        import evaluate_ucf101
        engines = []
        capsys.readouterr()
        res = evaluate_ucf101.iou('train', ["--ckpt", str(tmp_path)], hw=HW, on_engine=engines.append)
        out = capsys.readouterr().out
        assert len(res) == 2 and len(engines) == 1 and isinstance(engines[0], evalstep.EvalEngine) and engines[0].bs == 14
        direct = engines[0].evaluate(synthetic.make_eval_videos_u8(3, num_classes=24, hw=HW))      # the same engine, holding checkpoint b, called directly
        assert _same(res[0], res[1]) and _same(res[0], direct) and res[0]["n_tot_frames"].sum() > 0 and res[0]["n_vids"].sum() == 2
        assert out.count("Accuracy:") == 2 and "IoU/fmap/vmap" in out
        assert sorted(os.listdir(str(tmp_path))) == ["best_model_train_a.pth"]      # the tie goes to the first; the other is pruned
    finally:
        for k in list(sys.modules):
            if k in ("models", "utils", "evaluate_ucf101") or k.startswith(("models.", "utils.")):
                del sys.modules[k]
        sys.modules.update(saved)


def test_an_evaluation_pass_between_two_train_steps_changes_nothing(world):
    """Train step, evaluation pass on the step engine's weights, train step against the same two steps on a fresh engine: the second step's
    losses and the gradient of conv1.Mixed_4f.b1b.conv3d.weight are equal bit for bit, and so are the running statistics and the step count."""
    eng, ee = world["eng"], world["ee"]
    ref = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, evaluate_between in ((eng, True), (ref, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if evaluate_between:
            r = ee.evaluate(world["vids"])
            assert r["n_vids"].sum() == 3
            trained = r
            after_first = e.state_dict()                  # (read after the pass: results() has waited for the stream the pass ran on)
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
    # the pass evaluated the step engine's weights as the first train step left them (it waited for the step's lanes, not the host for the
    # step): an engine of its own holding that state gives the same tables
    own = evalstep.EvalEngine(bs=BS, hw=HW, state=after_first, capacity=64)
    assert _same(own.evaluate(world["vids"]), trained)
