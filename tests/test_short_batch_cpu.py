"""CPU: what lets the fused step run minibatches smaller than its planned size.
 - Plans for every n <= 8 bucket the gradient exactly as the plan for 8 does (data-parallel ranks whose steps differ in size must
   issue identical collectives) and keep its lane structure (FORK / JOIN sequence, the lane of every op);
 - the drop-in's synthetic loaders reproduce the epoch shape of the reference's DataLoaders (no drop_last, the labeled loader
   restarted when it runs out), and nothing changes when the new variables are unset;
 - the engine's minibatch check refuses what it cannot run."""
import os
import sys

import numpy as np
import pytest
import torch

from picons_amd import capi, spec, step as pstep
from picons_amd.plan import Plan
from tests.test_dropin_cpu import dropin_path  # noqa: F401  (fixture)

ARGS = pstep.default_args(bv=True, n_frames=5, wt_cons=0.1)


def _plan(n, jhmdb):
    p = Plan(21 if jhmdb else 24, 224, n=n, groups=2, training=True, jhmdb=jhmdb, lanes=4, early_adam=True)
    p.build_forward()
    p.build_loss(ARGS)
    p.build_backward()
    p.build_adam()
    p.finalize()
    return p


def _forks(p, name):
    return [(op[0], tuple(op[1][:2])) for op in p.lists[name] if op[0] in (capi.OP_FORK, capi.OP_JOIN)]


# The plan picks a conv's algorithm per launch shape (the bf16-split kernel where the library admits the shape, plan.maybe_x6) and
# folds split-K weight-gradient slices only where there is more than one: these are the ONLY kinds allowed to differ between sizes
_FAMILY = {capi.OP_CONV_X6: capi.OP_CONV}


def _shape(p, name):
    """Op-kind sequence (conv algorithm folded to one kind, slice folds left out) with every op's lane, FORK / JOIN with mask and source."""
    out = []
    for op in p.lists[name]:
        if op[0] in (capi.OP_FORK, capi.OP_JOIN):
            out.append((op[0], tuple(op[1][:2])))
        elif op[0] != capi.OP_WGRAD_FOLD:
            out.append((_FAMILY.get(op[0], op[0]), op[5]))
    return out


@pytest.fixture(scope="module")
def plans():
    return {(n, jh): _plan(n, jh) for jh in (False, True) for n in range(1, 9)}


@pytest.mark.parametrize("jhmdb", [False, True])
@pytest.mark.parametrize("n", range(1, 8))
def test_short_plan_buckets_and_lanes_match_full_plan(plans, n, jhmdb):
    full, p = plans[(8, jhmdb)], plans[(n, jhmdb)]
    assert p.poff == full.poff and p.roff == full.roff and p.nparams == full.nparams and p.adam_split == full.adam_split
    assert [b[1:] for b in p.grad_buckets(3_000_000)] == [b[1:] for b in full.grad_buckets(3_000_000)]
    assert [b[1:] for b in p.grad_buckets(3_000_000, joined=True)] == [b[1:] for b in full.grad_buckets(3_000_000, joined=True)]
    for name in ("fwd", "loss", "bwd", "adam"):
        assert _forks(p, name) == _forks(full, name), name
        assert _shape(p, name) == _shape(full, name), name
    # the early Adam op sits at the same place of the backward, on the same lane
    assert p.lists["bwd"][p.op_adam_early][5] == full.lists["bwd"][full.op_adam_early][5]


# ------------------------------------------------------------------------------------------------------------- drop-in loaders
def _sizes(loader):
    return [len(mb["action"]) for mb in loader]


def test_synthetic_loaders_follow_the_reference_epoch(dropin_path, monkeypatch):  # noqa: F811
    import main_ucf101 as M
    from torch.utils.data import DataLoader
    monkeypatch.setenv("PICONS_LABELED_CLIPS", "5")
    monkeypatch.setenv("PICONS_UNLABELED_CLIPS", "7")
    args = M.parse_args(["--bs", "4"])
    lab, unl, _val = M.synthetic_loaders(args, "1", 16)
    want_l = [len(b) for b in DataLoader(range(5), batch_size=2, shuffle=True)]
    want_u = [len(b) for b in DataLoader(range(7), batch_size=2, shuffle=True)]
    assert _sizes(lab) == want_l == [2, 2, 1] and len(lab) == 3
    assert _sizes(unl) == want_u == [2, 2, 2, 1] and len(unl) == 4
    mb = next(iter(lab))
    assert mb["data"].shape == (2, 3, spec.FRAMES, 16, 16) and mb["data"].dtype == torch.float64

    class Engine:             # records what train() hands the fused step
        def __init__(self):
            self.steps = []

        def train_step(self, label_mb, unlabel_mb, epoch, wt_ramp, perm, drops, lr=None, reducer=None):
            m = len(label_mb["action"]) + len(unlabel_mb["action"])
            assert sorted(perm) == list(range(m)) and all(d.shape[0] == m for d in drops)
            self.steps.append((len(label_mb["action"]), len(unlabel_mb["action"])))
            self.action_host, self._m = torch.zeros(m), m
            return dict(total=1.0, loc=0.5, cls=0.25, cons=0.25)

        def outputs(self):
            return None, None, torch.zeros(self._m, M.NUM_CLASSES)
    eng = Engine()
    model = torch.nn.Linear(1, 1)
    M.train(args, model, lab, unl, torch.optim.Adam(model.parameters(), lr=1e-3), 1, None, None, lambda e: 1.0, engine=eng)
    assert [a + b for a, b in eng.steps] == [4, 4, 3, 3]
    assert eng.steps == [(2, 2), (2, 2), (1, 2), (2, 1)]          # the labeled loader restarts at the fourth step


def test_synthetic_loaders_unchanged_without_the_variables(dropin_path, monkeypatch):  # noqa: F811
    import main_ucf101 as M
    monkeypatch.delenv("PICONS_LABELED_CLIPS", raising=False)
    monkeypatch.delenv("PICONS_UNLABELED_CLIPS", raising=False)
    monkeypatch.delenv("PICONS_STEPS", raising=False)
    args = M.parse_args(["--bs", "6"])
    lab, unl, val = M.synthetic_loaders(args, "1", 16)
    assert len(lab) == len(unl) == 4 and _sizes(lab) == _sizes(unl) == [3, 3, 3, 3]
    assert len(val) == 1 and _sizes(val) == [6]
    monkeypatch.setenv("PICONS_STEPS", "2")
    lab, unl, _ = M.synthetic_loaders(args, "1", 16)
    assert _sizes(lab) == _sizes(unl) == [3, 3]


def test_jhmdb_real_loaders_name_the_missing_module(dropin_path, monkeypatch):  # noqa: F811
    import main_ucf101 as M
    monkeypatch.setattr(M, "DATASET", "jhmdb")
    monkeypatch.setitem(sys.modules, "datasets", None)           # nothing importable under that name
    with pytest.raises(ImportError, match="datasets.load_jhmdb_pytorch_multi"):
        M.real_loaders(M.parse_args(["--bs", "4"]))


# ------------------------------------------------------------------------------------------------------------- minibatch check
def _engine_stub(bs, jhmdb=False):
    eng = pstep.StepEngine.__new__(pstep.StepEngine)          # the check reads bs / jhmdb only: no device needed
    eng.bs, eng.jhmdb = bs, jhmdb
    return eng


def _mb(n, labeled=True):
    return dict(data=np.zeros((n, 1)), aug_data=np.zeros((n, 1)), loc_msk=np.zeros((n, 1)), action=np.zeros((n, 1)),
                label_vid=(np.ones if labeled else np.zeros)(n))


def _drops(m):
    return [np.zeros((m, c), np.float32) for c in (spec.TRUNK_OUT_CH, 128, spec.TRUNK_OUT_CH, 128)]


def test_minibatch_check():
    eng = _engine_stub(4)
    assert eng.check_minibatch(_mb(2), _mb(2, False), np.arange(4)[::-1], _drops(4)) == (4, 2)
    assert eng.check_minibatch(_mb(1), _mb(2, False), np.array([2, 0, 1]), _drops(3)) == (3, 1)
    assert eng.check_minibatch(_mb(1), _mb(1, False), np.arange(2), _drops(2)) == (2, 1)
    bad = [
        (_mb(3), _mb(2, False), np.arange(5), _drops(5)),                        # more clips than the engine was built for
        (_mb(2), _mb(0, False), np.arange(2), _drops(2)),                        # no unlabeled clip
        (_mb(0), _mb(2, False), np.arange(2), _drops(2)),                        # no labeled clip
        (_mb(2), _mb(1, False), np.arange(4), _drops(3)),                        # perm of the wrong length
        (_mb(2), _mb(1, False), np.array([0, 1, 1]), _drops(3)),                 # not a permutation
        (_mb(2), _mb(1, False), np.arange(3), _drops(4)),                        # drops not (m, C)
        (_mb(2), _mb(1, False), np.arange(3), _drops(3)[:3]),                    # three drop arrays
        (dict(_mb(2), action=np.zeros((1, 1))), _mb(1, False), np.arange(3), _drops(3)),   # per-key sizes disagree
    ]
    for lab, unl, perm, drops in bad:
        with pytest.raises(ValueError):
            eng.check_minibatch(lab, unl, perm, drops)
    jh = _engine_stub(4, jhmdb=True)                           # JHMDB dicts need no label_vid (main_jhmdb.py:68-70)
    lab = {k: v for k, v in _mb(2).items() if k != "label_vid"}
    assert jh.check_minibatch(lab, lab, np.arange(4), _drops(4)) == (4, 2)
    with pytest.raises(ValueError):
        eng.check_minibatch(lab, lab, np.arange(4), _drops(4))


def test_dropin_builds_the_engine_for_the_largest_minibatch():
    """main_ucf101.run builds the engine for 2 * (bs // 2) clips: an odd --bs gives two loaders of bs // 2."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pi-consistency-activity-detection_amd", "dropin",
                            "main_ucf101.py")).read()
    assert "StepEngine(args, bs=2 * (args.bs // 2)" in src
