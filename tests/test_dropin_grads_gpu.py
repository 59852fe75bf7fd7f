"""GPU: the nn.Module drop-in's gradients, tensor by tensor.  The drop-in builds a plan the fused engine never builds
(`Plan(..., groups=1, accum_grads=True)`: one BatchNorm group, every gradient op ADDING into the flat buffer) and, used the reference's
way, replays its backward list twice per step.  Three checks:
 1. the two-pass step of test_dropin_gpu.py once more, every parameter judged by check_gradients_fp64_anchored (float64 oracle anchor);
 2. accumulation is addition: g(A + B) == g(A) + g(B) == g(A) then g(B) without zero_grad, per tensor, no oracle involved;
 3. the configurations no backward ran before: the 21-class head, an odd batch, the pseudo-label class mask (epoch >= thresh_ep)."""
import types

import pytest
import torch

from oracle import caps as ocaps, step as ostep
from picons_amd import model as pmodel, synthetic
from tests.test_step_gpu import check_gradients_fp64_anchored

pytestmark = pytest.mark.gpu

ADD_BAR = 1e-5      # part 2: an overwrite leaves an error of the size of one summand (ratio ~1); a second fp32 rounding where a gradient takes two adds a few 1e-7


def step_inputs(n_lab, n_unl, order, ncls, hw):
    """Clips, flipped clips and class indices of n_lab labeled + n_unl unlabeled synthetic clips, put in `order` (indices into labeled ++ unlabeled)."""
    if n_lab == n_unl:
        lab, unl, _, _ = synthetic.make_step_inputs(2 * n_lab, num_classes=ncls, hw=hw)
    else:
        lab, unl, _, _ = synthetic.make_step_inputs_split(n_lab, n_unl, num_classes=ncls, hw=hw)
    cat = lambda k: torch.cat([torch.from_numpy(lab[k]), torch.from_numpy(unl[k])])[order]
    return cat("data").float(), cat("aug_data").float(), cat("action")


def two_pass_loss(out, flip, pred):
    """Reaches every parameter from both passes."""
    return (out ** 2).mean() + (torch.flip(flip, [4]) - out).pow(2).mean() + pred.sum()


def oracle_two_pass(ncls, data, aug, action, labels, epoch, thresh_ep, d, dtype):
    """The oracle's two passes on the scripted dropout draws d (four {0, 2} scale tensors) -> (parameters with .grad, out, flip, pred, feat)."""
    n = data.shape[0]
    P = ostep.as_torch_params(synthetic.init_state(47, ncls), dtype=dtype)
    out, pred, feat = ocaps.capsnet_forward(P, data.to(dtype), action, labels, epoch, thresh_ep, True, d[0].view(n, 832).to(dtype), d[1].view(n, 128).to(dtype))
    flip, _, _ = ocaps.capsnet_forward(P, aug.to(dtype), action, labels, epoch, thresh_ep, True, d[2].view(n, 832).to(dtype), d[3].view(n, 128).to(dtype))
    two_pass_loss(out, flip, pred).backward()
    return P, out.detach(), flip.detach(), pred.detach(), feat.detach()


class Scripted:
    """torch.rand patched: records the module's dropout draws, or replays the ones given (forward of `data`: draws[0:2], of `aug`: draws[2:4])."""

    def __init__(self, replay=None):
        self.draws, self.replay = [], list(replay) if replay is not None else None

    def __enter__(self):
        self.orig = torch.rand

        def rand(*a, **k):
            if self.replay is not None:
                r = self.replay.pop(0)
                assert r.numel() == a[0]
                return r.to(k.get("device", "cpu"))
            r = self.orig(*a, **k)
            self.draws.append(r.detach().cpu())
            return r
        torch.rand = rand
        return self

    def __exit__(self, *exc):
        torch.rand = self.orig


class ModuleGrads:
    """What check_gradients_fp64_anchored reads of an engine: .plan.pshape and .grad(name)."""

    def __init__(self, m, grads):
        self.plan = types.SimpleNamespace(pshape=m._pshape)
        self.grads = grads

    def grad(self, name):
        return self.grads[name]


def grads_of(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def run_case(ncls, hw, n_lab, n_unl, order, labels, epoch, thresh_ep):
    """One module, the reference's two passes + one backward on recorded dropout draws, and the float32 / float64 oracle on the same draws."""
    torch.manual_seed(0)
    m = pmodel.CapsNet(pt_path=None, hw=hw, num_classes=ncls, init="conditioned").cuda()
    m.train(mode=True); m.training = True
    data, aug, action = step_inputs(n_lab, n_unl, order, ncls, hw)
    labels = torch.tensor(labels)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, eps=1e-6)
    opt.zero_grad()
    with Scripted() as rec:
        out, pred, feat = m(data.cuda(), action.cuda(), labels.cuda(), epoch, thresh_ep)
        flip, _, _ = m(aug.cuda(), action.cuda(), labels.cuda(), epoch, thresh_ep)
    two_pass_loss(out, flip, pred).backward()
    assert len(rec.draws) == 4
    d = [(x < 0.5).float() * 2 for x in rec.draws]
    c = types.SimpleNamespace(m=m, opt=opt, data=data, aug=aug, action=action, labels=labels, epoch=epoch, thresh_ep=thresh_ep, draws=rec.draws,
                              grads=grads_of(m), out=out.detach().cpu(), flip=flip.detach().cpu(), pred=pred.detach().cpu(), feat=feat.detach().cpu())
    c.P, c.o_out, c.o_flip, c.o_pred, c.o_feat = oracle_two_pass(ncls, data, aug, action, labels, epoch, thresh_ep, d, torch.float32)
    c.P64 = oracle_two_pass(ncls, data, aug, action, labels, epoch, thresh_ep, d, torch.float64)[0]
    return c


def check_case(c, tag):
    print("%s: max|d| vs the float32 oracle: out %.2e  flip %.2e  pred %.2e  feat %.2e" % (
        tag, (c.out - c.o_out).abs().max().item(), (c.flip - c.o_flip).abs().max().item(), (c.pred - c.o_pred).abs().max().item(),
        (c.feat - c.o_feat).abs().max().item()))
    assert (c.out - c.o_out).abs().max().item() <= 1e-3 and (c.pred - c.o_pred).abs().max().item() <= 1e-3
    assert (c.flip - c.o_flip).abs().max().item() <= 1e-3 and (c.feat - c.o_feat).abs().max().item() <= 5e-3
    dead = [k for k in c.m._pshape if not c.P64[k].grad.abs().max().item() > 0]
    assert not dead, "the loss does not reach %s" % dead[:10]
    rows = check_gradients_fp64_anchored(ModuleGrads(c.m, c.grads), c.P, c.P64, tag)
    name, rel_g, rel_c, _den = max(rows, key=lambda r: r[1] / max(4 * r[2], 5e-3))
    print("%s: worst tensor %s rel-L2 vs fp64 %.3e (fp32 oracle %.3e): %.2f of its bar" % (tag, name, rel_g, rel_c, rel_g / max(4 * rel_c, 5e-3)))


@pytest.fixture(scope="module")
def two_clips():
    """hw = 112, n = 2: the scenario of test_module_forward_backward_two_passes_vs_oracle."""
    return run_case(24, 112, 1, 1, [0, 1], [1, 0], 1, 11)


@pytest.fixture(scope="module")
def three_clips_jhmdb():
    """hw = 80, 21 classes (main_jhmdb.py), n = 3 (odd, one BatchNorm group), labeled / unlabeled / labeled, epoch 12 >= thresh_ep 11: the
    unlabeled clip's class mask is the argmax pseudo-label (mode 1 of pc_class_mask_fwd)."""
    return run_case(21, 80, 2, 1, [0, 2, 1], [1, 0, 1], 12, 11)


def test_two_pass_step_every_tensor_vs_fp64_oracle(two_clips):
    """Part 1.  Every one of the 293 gradients is the sum of two replays of the backward list into the flat buffer; each is held to
    rel-L2 <= max(4 x the float32 oracle's own distance from float64, 5e-3), so a bias or BatchNorm gradient that keeps only one pass's
    term fails by name however small it is next to the whole gradient."""
    check_case(two_clips, "dropin_n2_hw112")


def test_jhmdb_head_odd_batch_pseudo_label_mask_vs_fp64_oracle(three_clips_jhmdb):
    """Part 3.  Outputs and logits within 1e-3, feat within 5e-3 of the float32 oracle; every gradient by the rule of part 1."""
    c = three_clips_jhmdb
    assert c.m.num_classes == 21 and tuple(c.pred.shape) == (3, 21) and tuple(c.out.shape) == (3, 1, 8, 80, 80)
    check_case(c, "dropin_n3_hw80_c21")


def loss_a(out, pred):
    return (out ** 2).mean() + pred.sum()


def loss_b(out, pred):
    w = torch.linspace(0.5, 1.5, pred.shape[1], device=pred.device)
    return (torch.flip(out, [4]) - 1).pow(2).mean() + (pred * w).sum()


def test_accumulation_is_addition_per_tensor(two_clips):
    """Part 2.  Loss A on `data`, loss B on `aug`, the dropout draws replayed so that every forward of a clip set is the same function (batch
    statistics: the running ones do not enter).  gA, gB alone; gAB from one backward through both graphs; gSeq from two forward + backward
    pairs with no zero_grad between.  Per tensor max|gAB - (gA + gB)| and max|gSeq - (gA + gB)| <= 1e-5 max|gA + gB|: a replay that overwrites,
    or an add that is left out, errs by a whole summand; two adds instead of one round twice, a few 1e-7.  Then: zero_grad (grads None) and
    zero_grad(set_to_none=False) both start the next backward from zero."""
    c = two_clips
    m, opt = c.m, c.opt
    data, aug, action, labels = c.data.cuda(), c.aug.cuda(), c.action.cuda(), c.labels.cuda()

    def fwd_a():
        with Scripted(c.draws[0:2]):
            out, pred, _ = m(data, action, labels, c.epoch, c.thresh_ep)
        return loss_a(out, pred)

    def fwd_b():
        with Scripted(c.draws[2:4]):
            out, pred, _ = m(aug, action, labels, c.epoch, c.thresh_ep)
        return loss_b(out, pred)

    m.zero_grad(); fwd_a().backward(); gA = grads_of(m)
    m.zero_grad(); fwd_b().backward(); gB = grads_of(m)
    m.zero_grad(); (fwd_a() + fwd_b()).backward(); gAB = grads_of(m)
    m.zero_grad(); fwd_a().backward(); fwd_b().backward(); gSeq = grads_of(m)
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None for p in m.parameters())
    fwd_a().backward(); gA_zeroed = grads_of(m)
    opt.zero_grad()
    assert all(p.grad is None for p in m.parameters())
    fwd_a().backward(); gA_none = grads_of(m)

    vacuous, bad, worst = [], [], (-1.0, "", "")
    for k in m._pshape:
        na, nb = gA[k].norm().item(), gB[k].norm().item()
        if not (nb >= 1e-3 * na and na >= 1e-3 * nb and na > 0):
            vacuous.append((k, na, nb))
        s = gA[k] + gB[k]
        scale = s.abs().max().item()
        for what, got, ref, sc in (("one backward", gAB[k], s, scale), ("two backwards", gSeq[k], s, scale),
                                   ("zero_grad(set_to_none=False)", gA_zeroed[k], gA[k], gA[k].abs().max().item()),
                                   ("zero_grad()", gA_none[k], gA[k], gA[k].abs().max().item())):
            r = (got - ref).abs().max().item() / sc
            worst = max(worst, (r, k, what))
            if not r <= ADD_BAR:
                bad.append((k, what, r))
    inexact = sorted(k for k in m._pshape if not (torch.equal(gAB[k], gA[k] + gB[k]) and torch.equal(gSeq[k], gA[k] + gB[k])))
    print("additivity: worst max|got - sum| / max|sum| = %.3e (%s, %s); not bit-equal to gA + gB: %s" % (worst + (inexact,)))
    assert not vacuous, "one loss's gradient is negligible next to the other's: %s" % vacuous[:10]
    assert not bad, bad[:10]
