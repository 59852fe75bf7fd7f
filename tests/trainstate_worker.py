"""Resume equals uninterrupted, on the smallest engine the suite builds (bs 2, hw 112): used in-process by tests/test_trainstate_gpu.py and
as a child process for the data-parallel schedule (a one-rank RCCL group needs a process of its own):
    python tests/trainstate_worker.py reducer <tmpdir> <out.json>

A runs steps 0..3 in one go.  B runs steps 0 and 1 and its train_state() goes through trainstate.save / load.  C starts from ANOTHER seed's
weights, loads the file and runs steps 2 and 3.  B then loads the file itself (an engine that has already stepped), runs step 2, a
validation pass on its own ValEngine and step 3.  Every comparison is torch.equal: the step's gradients are bit-deterministic
(tests/test_wgrad_ordered_gpu.py), so a resumed run has no tolerance to hide in."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402
import picons_amd  # noqa: E402,F401
from picons_amd import step as pstep, synthetic, trainstate  # noqa: E402

HW, BS, LR, EPOCH = 112, 2, 1e-4, 1
LOSSES = ("total", "loc", "cls", "cons")


def make_args():
    return pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=LR, epochs=100)


def run_steps(eng, steps, reducer=None, between=None):
    """-> the four loss scalars of every step; between(): called between the steps."""
    ramp = pstep.exp_rampup(100)(EPOCH)
    out = []
    for n, i in enumerate(steps):
        if n and between is not None:
            between()
        lab, unl, perm, drops = synthetic.make_step_inputs(BS, rank=0, step=i, hw=HW)
        s = eng.train_step(lab, unl, EPOCH, ramp, perm, drops, lr=LR, reducer=reducer)
        out.append([s[k] for k in LOSSES])
    eng.synchronize()
    return out


def snapshot(eng):
    eng.synchronize()
    return dict(P=eng.P.clone(), R=eng.R.clone(), M=eng.M.clone(), V=eng.V.clone(), nbt=dict(eng.nbt), step_count=eng.step_count)


def same(a, b):
    """name -> equal?, for two snapshots."""
    r = {k: bool(torch.equal(a[k], b[k])) for k in ("P", "R", "M", "V")}
    r["nbt"] = a["nbt"] == b["nbt"]
    r["step_count"] = a["step_count"] == b["step_count"]
    return r


def max_diffs(a, b):
    return {k: float((a[k] - b[k]).abs().max()) for k in ("P", "R", "M", "V")}


def val_batch():
    return synthetic.make_minibatch(BS, True, 777, 24, HW)


def resume_world(tmpdir, reducer=False):
    """Runs A, B, C as described above; -> (results of plain types, engines and snapshots for further in-process checks)."""
    mk = lambda **kw: pstep.StepEngine(make_args(), bs=BS, hw=HW, device="cuda:0", **kw)
    A = mk()
    red = A.make_reducer(force=True) if reducer else None
    lossA = run_steps(A, range(4), red)
    snapA = snapshot(A)
    B = mk()
    redB = B.make_reducer(force=True) if reducer else None
    lossB = run_steps(B, range(2), redB)
    path = os.path.join(str(tmpdir), "engine_state.pt")
    trainstate.save(path, B.train_state())
    loaded = torch.load(path, map_location="cpu")
    C = mk(seed=53)
    redC = C.make_reducer(force=True) if reducer else None
    differs_before = not torch.equal(C.P, B.P)
    C.load_train_state(loaded)
    after_load = same(snapshot(C), snapshot(B))
    lossC = run_steps(C, (2, 3), redC)
    snapC = snapshot(C)
    # B again: loads its own file over its stepped state, and validates between the two remaining steps
    val = B.val_engine(BS)
    B.load_train_state(loaded)

    def val_pass():
        val.begin()
        val.val_step(val_batch())
        val.results()
    lossB2 = run_steps(B, (2, 3), redB, between=val_pass)
    snapB = snapshot(B)
    res = dict(reducer=bool(reducer), early_dp=[bool(r is not None and r.active) for r in (red, redB, redC)],
               last_adam_split=[A.last_adam_split, C.last_adam_split, A.plan.nparams],
               repeat_first_steps=lossA[:2] == lossB, differs_before=differs_before, after_load=after_load,
               state=same(snapA, snapC), state_diffs=max_diffs(snapA, snapC), losses_equal=lossA[2:] == lossC, lossA=lossA, lossC=lossC,
               state_with_val_pass=same(snapA, snapB), losses_with_val_pass=lossA[2:] == lossB2)
    return res, dict(A=A, B=B, C=C, snapA=snapA, loaded=loaded, val=val)


if __name__ == "__main__":
    mode, tmpdir, out = sys.argv[1], sys.argv[2], sys.argv[3]
    if mode == "reducer":
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        torch.distributed.init_process_group(backend="nccl", rank=0, world_size=1)
    res, _keep = resume_world(tmpdir, reducer=(mode == "reducer"))
    json.dump(res, open(out, "w"), indent=1)
    if mode == "reducer":
        torch.distributed.destroy_process_group()
