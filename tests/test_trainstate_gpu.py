"""GPU: StepEngine.train_state / load_train_state -- a resumed engine runs the very steps the uninterrupted one ran, bit for bit (plain and
through the data-parallel schedule), refusals change nothing, the optimiser state is torch.optim.Adam's own, and the engines that share
the step engine's buffers see the loaded weights.  All on the smallest engine the suite builds (bs 2, hw 112)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from picons_amd import model as pmodel, spec, step as pstep, trainstate, valstep
from tests import trainstate_worker as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    res, keep = W.resume_world(tmp_path_factory.mktemp("trainstate"))
    return dict(keep, res=res)


def _check(res):
    print(json.dumps({k: res[k] for k in ("state", "state_diffs", "lossA", "lossC", "after_load", "last_adam_split")}))
    assert res["differs_before"], "engine C must start from other weights, or the load proves nothing"
    assert all(res["after_load"].values()), res["after_load"]
    # A against its own repeat (B's first two steps): were this to fail, the step itself is not deterministic at this shape
    assert res["repeat_first_steps"], "two engines gave different losses for the same first two steps"
    assert all(res["state"].values()), (res["state"], res["state_diffs"])
    assert res["losses_equal"], (res["lossA"], res["lossC"])
    assert all(res["state_with_val_pass"].values()) and res["losses_with_val_pass"], res["state_with_val_pass"]


def test_resume_equals_uninterrupted(world):
    """P, R, M, V, num_batches_tracked, the step count and the four loss scalars of steps 2 and 3: equal between the engine that ran steps
    0..3 and the one that loaded the state after step 1 into another seed's engine; and the same with a validation pass between the two
    steps after the load."""
    _check(world["res"])
    assert world["res"]["last_adam_split"][0] < world["res"]["last_adam_split"][2]         # the early Adam op ran, with the loaded count


def test_resume_equals_uninterrupted_data_parallel(tmp_path):
    """The same through a one-rank RCCL group (segmented backward, bucket all-reduces, arm_early_adam_dp's step count after a load)."""
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    out = str(tmp_path / "dp.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trainstate_worker.py"), "reducer", str(tmp_path), out], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and os.path.exists(out), p.stdout[-3000:]
    res = json.load(open(out))
    assert res["reducer"] and all(res["early_dp"])
    _check(res)


def _frozen(eng):
    eng.synchronize()
    return eng.P.clone(), eng.M.clone(), eng.V.clone(), eng.step_count


def test_refusals_change_nothing(world):
    C = world["C"]
    before = _frozen(C)

    def refused(state, match):
        with pytest.raises(ValueError, match=match):
            C.load_train_state(state)
        now = _frozen(C)
        assert all(torch.equal(a, b) for a, b in zip(before[:3], now[:3])) and before[3] == now[3]

    good = world["loaded"]
    names = C.param_names()
    last = len(names) - 1                                  # the last tensor: everything before it has passed by the time it is refused
    bad = dict(good, optimizer=dict(good["optimizer"], state={i: dict(s) for i, s in good["optimizer"]["state"].items()}))
    bad["optimizer"]["state"][last]["exp_avg"] = torch.zeros(tuple(C.plan.pshape[names[last]]) + (2,))
    refused(bad, names[last].replace(".", r"\."))
    bad = dict(good, model=dict(good["model"]))
    bad["model"][names[last]] = torch.zeros(tuple(C.plan.pshape[names[last]]) + (2,))
    refused(bad, names[last].replace(".", r"\."))
    bad = dict(good, step_count=good["step_count"] + 1)
    refused(bad, "step_count")
    refused({"model": good["model"]}, "optimizer")
    # a 21-class state into this 24-class engine (no GPU work: the state is made on the host)
    from picons_amd.plan import Plan
    from picons_amd import synthetic
    lay = Plan(21, W.HW, n=1, groups=1)
    n21 = [k for k in spec.state_dict_keys(21) if k in lay.pshape]
    M21 = torch.ones(lay.nparams)
    st21 = {"model": {k: torch.as_tensor(np.asarray(v)) for k, v in synthetic.init_state(47, 21).items()},
            "optimizer": trainstate.adam_state_from_flat(M21, M21, 2, lay.poff, lay.pshape, n21, [trainstate.adam_param_group(1e-4)]), "step_count": 2}
    refused(st21, "shape")


def test_parameter_order_is_named_parameters(world):
    eng = world["C"]
    net = pmodel.CapsNet(pt_path=None, hw=W.HW)
    assert eng.param_names() == [k for k in spec.state_dict_keys(24) if k in eng.plan.pshape] == [n for n, _ in net.named_parameters()]


def test_interop_with_torch_adam(world):
    """After fused steps the optimiser state loads into the drop-in module's own torch.optim.Adam, tensor for tensor the engine's slices; that
    optimiser's state_dict() loaded back reproduces M, V and the step count."""
    eng = world["A"]
    ts = eng.train_state()
    assert ts["step_count"] == 4 and list(ts["model"]) == spec.state_dict_keys(24) and not any(v.is_cuda for v in ts["model"].values())
    g = ts["optimizer"]["param_groups"][0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (W.LR, (0.9, 0.999), 1e-6, 0)
    net = pmodel.CapsNet(pt_path=None, hw=W.HW)
    opt = torch.optim.Adam(net.parameters(), eps=1e-6)
    opt.load_state_dict(ts["optimizer"])
    for (name, p) in net.named_parameters():
        o, n = eng.plan.poff[name], p.numel()
        assert torch.equal(opt.state[p]["exp_avg"].reshape(-1), eng.M[o:o + n]) and torch.equal(opt.state[p]["exp_avg_sq"].reshape(-1), eng.V[o:o + n]), name
        assert float(opt.state[p]["step"]) == 4
    back = pstep.StepEngine(W.make_args(), bs=W.BS, hw=W.HW, seed=59)
    back.load_train_state({"model": ts["model"], "optimizer": opt.state_dict()})
    back.synchronize()
    assert torch.equal(back.M, eng.M) and torch.equal(back.V, eng.V) and back.step_count == 4 and torch.equal(back.P, eng.P) and torch.equal(back.R, eng.R)


def test_other_engines_see_the_loaded_weights(world):
    """A ValEngine made from the step engine BEFORE the load reads the loaded weights (its weight layouts are made per pass): one forward,
    bitwise against an engine built from the same model state."""
    B, val, loaded = world["B"], world["val"], world["loaded"]
    B.load_train_state(loaded)
    mb = W.val_batch()
    val.begin()
    val.val_step(mb)
    got = val.results()
    out, pred = (t.clone() for t in val.outputs())
    own = valstep.ValEngine(W.BS, hw=W.HW, state=loaded["model"])
    own.begin()
    own.val_step(mb)
    want = own.results()
    out2, pred2 = own.outputs()
    assert torch.equal(out, out2) and torch.equal(pred, pred2)
    assert got[0]["total"] == want[0]["total"] and np.array_equal(got[0]["counts"], want[0]["counts"])
