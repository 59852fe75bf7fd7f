"""CPU: picons_amd.trainstate -- the training-state format, the conversions between flat Adam moment buffers and the per-tensor state
torch.optim.Adam.state_dict() writes, and every refusal; none of it needs a GPU."""
import os
import sys

import pytest
import torch

from picons_amd import trainstate as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPIN = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin")

# four tensors with gaps between them (and in front of the first and behind the last) in flat buffers of 64 floats
PSHAPE = {"a.weight": (2, 3), "a.bias": (3,), "b.weight": (4, 1, 2), "c.scalar": (1,)}
POFF = {"a.weight": 2, "a.bias": 10, "b.weight": 17, "c.scalar": 40}
NAMES = list(PSHAPE)
NFLAT = 64
GAPS = [i for i in range(NFLAT) if not any(POFF[k] <= i < POFF[k] + int(torch.tensor(PSHAPE[k]).prod()) for k in NAMES)]


def _flat(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(NFLAT, generator=g) + 0.5, torch.rand(NFLAT, generator=g) + 0.5


def _real_adam(steps=1):
    params = [torch.nn.Parameter(torch.ones(PSHAPE[k])) for k in NAMES]
    opt = torch.optim.Adam(params, lr=1e-3, eps=1e-6, weight_decay=0)
    for _ in range(steps):
        for p in params:
            p.grad = torch.full_like(p, 0.25)
        opt.step()
    return params, opt


def _state(step=7, seed=1):
    M, V = _flat(seed)
    return M, V, ts.adam_state_from_flat(M, V, step, POFF, PSHAPE, NAMES, [ts.adam_param_group(1e-3)])


def test_round_trip_leaves_the_gaps_alone():
    M, V, sd = _state(step=7)
    M2, V2 = torch.full((NFLAT,), -3.0), torch.full((NFLAT,), -5.0)
    assert ts.adam_state_to_flat(sd, M2, V2, POFF, PSHAPE, NAMES) == 7
    for k in NAMES:
        o, n = POFF[k], sd["state"][NAMES.index(k)]["exp_avg"].numel()
        assert torch.equal(M2[o:o + n], M[o:o + n]) and torch.equal(V2[o:o + n], V[o:o + n]), k
        assert tuple(sd["state"][NAMES.index(k)]["exp_avg"].shape) == PSHAPE[k]
    assert len(GAPS) == NFLAT - 18
    assert torch.all(M2[GAPS] == -3.0) and torch.all(V2[GAPS] == -5.0)
    # the produced tensors are copies: writing the flat buffers afterwards does not reach them
    M.zero_()
    assert float(sd["state"][0]["exp_avg"].abs().sum()) > 0
    # a count of zero is a fresh optimiser: no state, and loading it clears the moments of every named tensor
    fresh = ts.adam_state_from_flat(M, V, 0, POFF, PSHAPE, NAMES, [ts.adam_param_group(1e-3)])
    assert fresh["state"] == {}
    assert ts.adam_state_to_flat(fresh, M2, V2, POFF, PSHAPE, NAMES) == 0
    assert torch.all(M2[GAPS] == -3.0) and float(M2[POFF["b.weight"]:POFF["b.weight"] + 8].abs().sum()) == 0


def test_format_is_torch_adams_own():
    _, _, sd = _state(step=1)
    params, opt = _real_adam(1)
    own = opt.state_dict()
    assert set(sd) == set(own) and set(sd["state"]) == set(own["state"])
    assert set(sd["param_groups"][0]) == set(own["param_groups"][0]) and sd["param_groups"][0]["params"] == own["param_groups"][0]["params"]
    for i in own["state"]:
        assert set(sd["state"][i]) == set(own["state"][i])
        for k, v in own["state"][i].items():
            assert type(sd["state"][i][k]) is type(v), k
            assert sd["state"][i][k].dtype == v.dtype and sd["state"][i][k].shape == v.shape, (i, k)
    assert float(sd["state"][0]["step"]) == 1.0
    _, fresh = _real_adam(0)
    fresh.load_state_dict(sd)
    got = fresh.state_dict()
    for i in sd["state"]:
        for k in sd["state"][i]:
            assert torch.equal(got["state"][i][k], sd["state"][i][k])
    # and back: a real Adam's state goes into flat buffers
    M2, V2 = torch.zeros(NFLAT), torch.zeros(NFLAT)
    assert ts.adam_state_to_flat(own, M2, V2, POFF, PSHAPE, NAMES) == 1
    assert torch.allclose(M2[POFF["a.bias"]:POFF["a.bias"] + 3], torch.full((3,), 0.025))


def _refused(sd, match, names=NAMES):
    M, V = _flat(9)
    m0, v0 = M.clone(), V.clone()
    with pytest.raises(ValueError, match=match):
        ts.adam_state_to_flat(sd, M, V, POFF, PSHAPE, names)
    assert torch.equal(M, m0) and torch.equal(V, v0)


def test_refusals_write_nothing():
    _, _, sd = _state()
    del sd["state"][3]
    _refused(sd, "3 tensors.*4 parameters.*c.scalar")
    _, _, sd = _state()
    sd["state"][4] = dict(sd["state"][0])
    _refused(sd, "5 tensors")
    # the LAST tensor is the bad one: everything before it has passed its checks and must still not be written
    _, _, sd = _state()
    sd["state"][2]["exp_avg_sq"] = torch.zeros(4, 2, 1)
    _refused(sd, "b.weight.*exp_avg_sq.*\\(4, 2, 1\\)")
    _, _, sd = _state()
    sd["state"][3]["step"] = torch.tensor(8.0)
    _refused(sd, "c.scalar.*step 8.*step 7")
    for bad in (float("nan"), float("inf")):
        _, _, sd = _state()
        sd["state"][3]["exp_avg"][0] = bad
        _refused(sd, "c.scalar.*exp_avg.*non-finite")
        _, _, sd = _state()
        sd["state"][1]["exp_avg_sq"][2] = bad
        _refused(sd, "a.bias.*exp_avg_sq.*non-finite")
    _, _, sd = _state()
    sd["state"][0]["step"] = torch.tensor(float("nan"))
    _refused(sd, "a.weight.*step")
    _refused({"state": None}, "optimizer state")


def test_model_state_of():
    bare = {"w": torch.ones(2), "bn.num_batches_tracked": torch.tensor(3)}
    assert ts.model_state_of(bare) is bare
    full = {"format": ts.FORMAT, "version": ts.VERSION, "model": bare, "optimizer": {}}
    assert ts.model_state_of(full) is bare
    with pytest.raises(ValueError, match="format 'something_else'"):
        ts.model_state_of(dict(full, format="something_else"))
    with pytest.raises(ValueError, match="version 2"):
        ts.model_state_of(dict(full, version=ts.VERSION + 1))
    with pytest.raises(ValueError, match="neither a state_dict nor.*model.*optimizer"):
        ts.model_state_of({"model": bare, "optimizer": {"state": {}}})
    with pytest.raises(ValueError, match="neither"):
        ts.model_state_of({})
    with pytest.raises(ValueError, match="list"):
        ts.model_state_of([bare])


def _small_state():
    _, _, opt = _state(step=2)
    return {"format": ts.FORMAT, "version": ts.VERSION, "model": {"w": torch.arange(4.0)}, "optimizer": opt,
            "scheduler": {"best": 1.5, "num_bad_epochs": 2}, "epoch": 3,
            "best": dict(val_loss=1.5, train_loss=2.5, val_path="d/v.pth", train_path=None, save_dir="d"),
            "rng": ts.rng_state(), "args": dict(epochs=100, lr=1e-4, bv=True, lower_thresh=None),
            "meta": dict(num_classes=24, hw=224, dataset="ucf101", world=1, fused=True)}


def test_save_is_atomic_and_load_round_trips(tmp_path, monkeypatch):
    path = str(tmp_path / "state.pt")
    st = _small_state()
    ts.save(path, st)
    assert sorted(os.listdir(str(tmp_path))) == ["state.pt"]
    before = open(path, "rb").read()
    got = ts.load(path)
    assert got["epoch"] == 3 and got["best"] == st["best"] and got["args"] == st["args"] and got["meta"] == st["meta"]
    assert torch.equal(got["model"]["w"], st["model"]["w"]) and torch.equal(got["optimizer"]["state"][2]["exp_avg"], st["optimizer"]["state"][2]["exp_avg"])
    assert got["optimizer"]["param_groups"] == st["optimizer"]["param_groups"] and got["scheduler"] == st["scheduler"]

    real_save = torch.save

    def failing(obj, f, *a, **k):
        real_save({"half": torch.zeros(3)}, f)          # the temporary file exists by the time the write fails
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", failing)
    with pytest.raises(OSError, match="disk full"):
        ts.save(path, dict(st, epoch=4))
    monkeypatch.setattr(torch, "save", real_save)
    assert sorted(os.listdir(str(tmp_path))) == ["state.pt"] and open(path, "rb").read() == before

    torch.save({"w": torch.ones(2)}, str(tmp_path / "bare.pth"))
    with pytest.raises(ValueError, match="not a picons_train_state"):
        ts.load(str(tmp_path / "bare.pth"))
    short = dict(st)
    del short["scheduler"]
    ts.save(str(tmp_path / "short.pt"), short)
    with pytest.raises(ValueError, match="lacks.*scheduler"):
        ts.load(str(tmp_path / "short.pt"))


def test_rng_state_round_trips_through_a_file(tmp_path):
    import random
    import numpy as np
    random.seed(5); np.random.seed(6); torch.manual_seed(7)
    path = str(tmp_path / "s.pt")
    ts.save(path, dict(_small_state(), rng=ts.rng_state()))
    want = (random.random(), np.random.rand(3).tolist(), torch.rand(3), torch.randperm(5))
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    ts.set_rng_state(ts.load(path)["rng"], rank=0)
    got = (random.random(), np.random.rand(3).tolist(), torch.rand(3), torch.randperm(5))
    assert got[:2] == want[:2] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    with pytest.raises(ValueError, match="rank 1"):
        ts.set_rng_state(ts.load(path)["rng"], rank=1)


def test_check_compatible():
    st = _small_state()
    meta = dict(st["meta"])
    assert ts.check_compatible(st, meta, dict(st["args"])) == []
    for k, other in (("num_classes", 21), ("hw", 112), ("dataset", "jhmdb"), ("world", 2)):
        with pytest.raises(ValueError, match=k):
            ts.check_compatible(st, dict(meta, **{k: other}), dict(st["args"]))
    assert ts.check_compatible(st, dict(meta, fused=False), dict(st["args"])) == []
    diffs = ts.check_compatible(st, meta, dict(st["args"], epochs=120))
    assert diffs == [("epochs", 100, 120)]
    text = ts.arg_warning(diffs)
    assert "--epochs 120" in text and "exp_rampup" in text and "ramp" in text
    assert "exp_rampup" not in ts.arg_warning([("lr", 1e-4, 1e-3)])


@pytest.fixture()
def dropin_path():
    names = ("models", "utils", "main_ucf101", "main_jhmdb")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in names or k.startswith(("models.", "utils."))}
    sys.path.insert(0, DROPIN)
    yield
    sys.path.remove(DROPIN)
    for k in list(sys.modules):
        if k in names or k.startswith(("models.", "utils.")):
            del sys.modules[k]
    sys.modules.update(saved)


def test_cli_surface_has_no_resume_flag(dropin_path):
    """Checkpointing is switched by the environment alone: both parsers keep the reference's flag set."""
    import main_ucf101 as M
    import main_jhmdb as J
    a, j = M.parse_args([]), J.parse_args([])
    assert sorted(vars(a)) == sorted(
        "bs epochs model_name lr pf pretrained loc_loss exp_id pkl_file_label pkl_file_unlabel const_loss wt_loc wt_cls wt_cons seed "
        "thresh_epoch workers n_frames bv predict_maps bv_wt cyclic gv lower_thresh upper_thresh gv_wt".split())
    assert (a.bs, a.epochs, a.lr, a.seed, a.exp_id) == (16, 1, 0.001, 47, "debug") and (j.bs, j.epochs, j.wt_seg, j.seed_num) == (16, 1, 1, 47)
    for ns in (a, j):
        assert not hasattr(ns, "resume") and not any("resume" in k or "state" in k for k in vars(ns))
    assert callable(M.write_train_state) and callable(M.restore_train_state) and not hasattr(J, "write_train_state")
