"""GPU: the drop-in trainer resumes a run bit for bit at an epoch boundary (PICONS_TRAIN_STATE / PICONS_EPOCHS_THIS_RUN / PICONS_RESUME).
Child processes of dropin/main_ucf101.py on synthetic minibatches at 112 px, two epochs of two steps:
  (a) straight through;  (b) the same, stopped after epoch 1;  (c) resumed from (b)'s file, in a working directory of its own.
(a) and (c) must leave the same training state, the same checkpoints and -- for (c) -- only epoch 2 on stdout."""
import os
import subprocess
import sys

import pytest
import torch

from picons_amd import model as pmodel, trainstate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin")
HW = 112
FLAGS = ["--bs", "4", "--epochs", "2", "--bv", "--n_frames", "5", "--exp_id", "r"]


def _start(script, cwd, **env):
    os.makedirs(cwd, exist_ok=True)
    e = dict(os.environ, PICONS_SYNTHETIC="1", PICONS_HW=str(HW), PICONS_STEPS="2", **env)
    for k in ("PICONS_TRAIN_STATE", "PICONS_RESUME", "PICONS_EPOCHS_THIS_RUN", "PICONS_FUSED"):
        if k not in env:
            e.pop(k, None)
    return subprocess.Popen([sys.executable, os.path.join(DROPIN, script)] + FLAGS, cwd=cwd, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(p, limit=600):
    out, err = p.communicate(timeout=limit)
    assert p.returncode == 0, (out[-1500:], err[-3000:])
    return out


def _ckpts(state):
    d = state["best"]["save_dir"]
    return d, sorted(f for f in os.listdir(d) if f.startswith("best_model_"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    top = str(tmp_path_factory.mktemp("resume"))
    dirs = {k: os.path.join(top, k) for k in "abcd"}
    files = {k: os.path.join(top, "state_%s.pt" % k) for k in "ab"}
    pa = _start("main_ucf101.py", dirs["a"], PICONS_TRAIN_STATE=files["a"])
    pb = _start("main_ucf101.py", dirs["b"], PICONS_TRAIN_STATE=files["b"], PICONS_EPOCHS_THIS_RUN="1")
    out = {"a": _finish(pa), "b": _finish(pb)}
    after_b = trainstate.load(files["b"])
    assert after_b["epoch"] == 1 and "[VAL] epoch-1" in out["b"] and "[VAL] epoch-2" not in out["b"]
    out["c"] = _finish(_start("main_ucf101.py", dirs["c"], PICONS_RESUME=files["b"], PICONS_TRAIN_STATE=files["b"]))
    return dict(dirs=dirs, files=files, out=out, after_b=after_b, a=trainstate.load(files["a"]), c=trainstate.load(files["b"]))


def _same_tree(x, y, where="state"):
    if torch.is_tensor(x):
        assert torch.is_tensor(y) and x.dtype == y.dtype and torch.equal(x, y), where
    elif isinstance(x, dict):
        assert isinstance(y, dict) and list(x) == list(y), where
        for k in x:
            _same_tree(x[k], y[k], "%s[%r]" % (where, k))
    elif isinstance(x, (list, tuple)):
        assert len(x) == len(y), where
        for i, (u, v) in enumerate(zip(x, y)):
            _same_tree(u, v, "%s[%d]" % (where, i))
    else:
        assert x == y, (where, x, y)


def test_resumed_run_equals_the_uninterrupted_one(runs):
    a, c = runs["a"], runs["c"]
    assert a["epoch"] == c["epoch"] == 2
    assert a["optimizer"]["state"] and float(a["optimizer"]["state"][0]["step"]) == 4.0
    _same_tree(a["model"], c["model"], "model")
    _same_tree(a["optimizer"], c["optimizer"], "optimizer")
    _same_tree(a["scheduler"], c["scheduler"], "scheduler")
    _same_tree(a["rng"], c["rng"], "rng")
    base = lambda p: None if p is None else os.path.basename(p)
    for k in ("val_loss", "train_loss"):
        assert a["best"][k] == c["best"][k], k
    for k in ("val_path", "train_path"):
        assert base(a["best"][k]) == base(c["best"][k]), k
    # (c) went on in (b)'s checkpoint directory, not in one of its own
    assert c["best"]["save_dir"] == runs["after_b"]["best"]["save_dir"] and c["best"]["save_dir"].startswith(runs["dirs"]["b"])
    assert not os.path.exists(os.path.join(runs["dirs"]["c"], "train_log_wts"))
    (da, fa), (dc, fc) = _ckpts(a), _ckpts(c)
    assert fa == fc and fa
    for f in fa:
        _same_tree(torch.load(os.path.join(da, f), map_location="cpu"), torch.load(os.path.join(dc, f), map_location="cpu"), f)
    assert "[VAL] epoch-2" in runs["out"]["c"] and "epoch-1" not in runs["out"]["c"]
    assert "[VAL] epoch-1" in runs["out"]["a"] and "[VAL] epoch-2" in runs["out"]["a"]


def test_finished_run_is_not_trained_again(runs):
    """A state whose epoch is --epochs: exit 0, a message, no training and no checkpoint directory."""
    out = _finish(_start("main_ucf101.py", runs["dirs"]["d"], PICONS_RESUME=runs["files"]["a"]))
    assert "nothing left to train" in out and "[VAL]" not in out and "Training time" not in out
    assert not os.path.exists(os.path.join(runs["dirs"]["d"], "train_log_wts"))


def test_load_previous_weights_reads_a_training_state(runs, tmp_path):
    a = runs["a"]
    d, files = _ckpts(a)
    last = [f for f in files if f.endswith("_2.pth")]
    want = torch.load(os.path.join(d, last[0]), map_location="cpu") if last else a["model"]
    net = pmodel.CapsNet(pt_path=None, hw=HW, seed=5)
    net.load_previous_weights(runs["files"]["a"])
    got = net.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k].cpu(), want[k]) for k in want)
    _same_tree(a["model"], {k: v.cpu() for k, v in got.items()}, "model")
    bad = str(tmp_path / "wrapped.pth")
    torch.save({"model": a["model"], "optimizer": a["optimizer"]}, bad)
    before = {k: v.clone() for k, v in got.items()}
    with pytest.raises(ValueError, match="neither a state_dict nor"):
        net.load_previous_weights(bad)
    assert all(torch.equal(before[k], v) for k, v in net.state_dict().items())
