"""GPU: valstep.ValEngine (the validation pass on the device) at hw = 112, as the other drop-in tests.  The metric is checked apart from
the network (the records against torch losses and the drop-in's IOU2 on the engine's own outputs), the network against
CapsNet.eval() holding the same weights, the drop-in's validate(..., engine=...) against validate(...), and a validation pass between
two train steps must leave the second step bit for bit what it is without the pass."""
import os
import sys

import numpy as np
import pytest
import torch

from picons_amd import model as pmodel, ops, step as pstep, synthetic, valstep

pytestmark = pytest.mark.gpu
HW = 112
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin")
_NAMES = ("models", "utils", "main_ucf101", "main_jhmdb")


def _args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)


def _batches():
    return [{k: torch.from_numpy(v) for k, v in synthetic.make_minibatch(n, True, 4100 + n, 24, HW).items() if k in valstep.KEYS} for n in (3, 2)]


@pytest.fixture(scope="module")
def dropin():
    """dropin/main_ucf101.py imported the way its users run it (its directory first on sys.path), with the module globals validate reads."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in _NAMES or k.startswith(("models.", "utils."))}
    sys.path.insert(0, DROPIN)
    import main_ucf101 as M
    yield M
    sys.path.remove(DROPIN)
    for k in list(sys.modules):
        if k in _NAMES or k.startswith(("models.", "utils.")):
            del sys.modules[k]
    sys.modules.update(saved)


@pytest.fixture(scope="module")
def world(dropin):
    """One StepEngine(bs=2) with its val_engine(3), one pass over batches of 3, 2 and again the 3 clips, and CapsNet.eval() on the same weights:
    computed once and shared by the tests below.  Only the last test of the file trains the engine; the others leave everything as it is."""
    M = dropin
    eng = pstep.StepEngine(_args(), bs=2, hw=HW)
    ve = eng.val_engine(3)
    batches = _batches()
    ve.begin()
    outs = []
    for mb in batches + batches[:1]:
        ve.val_step(mb)
        out, pred = ve.outputs()
        outs.append((out.clone(), pred.clone()))
    recs = ve.results()
    net = pmodel.CapsNet(pt_path=None, hw=HW, init="conditioned").cuda()
    net.load_state_dict(eng.state_dict())
    net.eval(); net.training = False
    M.model = net
    M.criterion_cls = M.SpreadLoss(num_class=24, m_min=0.2, m_max=0.9)
    M.criterion_seg_1 = torch.nn.BCEWithLogitsLoss()
    M.criterion_seg_2 = M.DiceLoss()
    return dict(M=M, eng=eng, ve=ve, batches=batches, outs=outs, recs=recs, net=net)


def test_records_equal_torch_losses_and_iou2_on_the_engines_outputs(world):
    M = world["M"]
    for mb, (out, pred), r in zip(world["batches"], world["outs"], world["recs"]):
        seg = mb["loc_msk"].cuda().float()
        act = mb["action"].cuda()
        cls, _abs = M.criterion_cls(pred, act)
        loc = M.criterion_seg_1(out, seg) + M.criterion_seg_2(out, seg)
        print("val record B=%d: total %.7f / torch %.7f  loc %.7f / %.7f  cls %.7f / %.7f" % (r["B"], r["total"], float(loc + cls), r["loc"], float(loc), r["cls"], float(cls)))
        assert abs(r["loc"] - float(loc)) <= 1e-4 and abs(r["cls"] - float(cls)) <= 1e-4 and abs(r["total"] - float(loc + cls)) <= 1e-4
        assert r["n_correct"] / r["B"] == M.get_accuracy(pred, act)
        mask = (out.cpu().numpy() > 0).astype(np.float32)
        truth = seg.cpu().numpy()
        for a in range(r["B"]):
            inter, union, gt = r["counts"][a].tolist()
            s = truth[a] + mask[a]
            assert (inter, union, gt) == (int((s >= 2).sum()), int(np.minimum(s, 1).sum()), int(truth[a].sum()))
            assert gt > 0 and float(inter) / float(union) == M.IOU2(truth[a], mask[a])


def test_weight_layouts_made_once_per_pass_serve_every_batch(world):
    """The third batch is the first again, run after another plan's batch on layouts made before the first: the same record, bit for bit."""
    a, b = world["recs"][0], world["recs"][2]
    assert all(a[k] == b[k] for k in ops.VAL_SCALARS) and a["n_correct"] == b["n_correct"] and np.array_equal(a["counts"], b["counts"])
    assert torch.equal(world["outs"][0][0], world["outs"][2][0]) and torch.equal(world["outs"][0][1], world["outs"][2][1])


def test_outputs_match_capsnet_eval_on_the_same_weights(world):
    net = world["net"]
    for mb, (out, pred) in zip(world["batches"], world["outs"]):
        n = len(mb["action"])
        with torch.no_grad():
            o, p, _ = net(mb["data"].float().cuda(), mb["action"].cuda(), torch.zeros(n).cuda(), 0, 0)
        d_o, d_p = (o - out).abs().max().item(), (p - pred).abs().max().item()
        print("val engine vs CapsNet.eval: |dlogits| %.2e |dscores| %.2e" % (d_o, d_p))
        assert d_o <= 1e-3 and d_p <= 1e-3


def test_dropin_validate_with_and_without_engine(world, capsys):
    M = world["M"]
    capsys.readouterr()
    base = M.validate(world["net"], world["batches"], 3)
    line0 = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VAL]")]
    got = M.validate(world["net"], world["batches"], 3, world["ve"])
    line1 = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[VAL]")]
    print(line0, line1, base, got)
    assert abs(base - got) <= 1e-4
    assert len(line0) == 1 and line0 == line1                      # the three printed decimals of loss, accuracy and IoU


def test_bad_minibatches_raise_before_anything_is_enqueued(world):
    ve = world["ve"]
    good = world["batches"][1]
    ve.begin()
    state = (ve.k, ve.slot, list(ve.used), ve.table.clone())
    for bad in (dict(good, action=torch.tensor([[0.0], [24.0]])), dict(good, action=torch.tensor([[-1.0], [3.0]])), dict(good, action=torch.tensor([[1.5], [3.0]])),
                {k: v for k, v in good.items() if k != "loc_msk"}, {k: v for k, v in good.items() if k != "data"},
                dict(good, data=good["data"][:, :, :, :HW - 8]), dict(good, data=good["data"][:, :, :4]), dict(good, loc_msk=good["loc_msk"][:1]),
                dict(good, action=good["action"][:1]), {k: torch.cat([v, v]) for k, v in good.items()}):
        with pytest.raises(ValueError):
            ve.val_step(bad)
        assert (ve.k, ve.slot, list(ve.used)) == state[:3]
    assert torch.equal(ve.table, state[3]) and ve.results() == []


def test_a_validation_pass_between_two_train_steps_changes_nothing(world):
    """Train step, validation pass, train step on the shared engine against the same two steps on a fresh engine: the second step's losses
    and the gradient of conv1.Mixed_4f.b1b.conv3d.weight are equal bit for bit, and so are the running statistics and the step count."""
    eng, ve = world["eng"], world["ve"]
    ref = pstep.StepEngine(_args(), bs=2, hw=HW)
    ramp = pstep.exp_rampup(100)(1)
    name = "conv1.Mixed_4f.b1b.conv3d.weight"
    res = []
    for e, validate_between in ((eng, True), (ref, False)):
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=0, hw=HW)
        e.train_step(lab, unl, 1, ramp, perm, drops)
        if validate_between:
            ve.begin()
            for mb in world["batches"]:
                ve.val_step(mb)
            assert len(ve.results()) == 2
        lab, unl, perm, drops = synthetic.make_step_inputs(2, rank=0, step=1, hw=HW)
        losses = e.train_step(lab, unl, 1, ramp, perm, drops)
        e.synchronize()
        res.append((losses, e.grad(name).clone(), e.R.clone(), e.step_count, dict(e.nbt)))
    (l0, g0, r0, s0, n0), (l1, g1, r1, s1, n1) = res
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1) and torch.equal(r0, r1) and s0 == s1 == 2 and n0 == n1
