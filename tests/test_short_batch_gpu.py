"""GPU: the fused step on minibatches smaller than the engine's planned size (the reference's loaders end each epoch on a short
batch, main_ucf101.py:353-366, and an odd --bs gives bs - 1 clips per step).  Every case runs in a process of its own under a time
limit (tests/short_batch_worker.py holds the checks); the drop-in case runs the training script over a stand-in for the caller's
dataset module."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "short_batch_worker.py")
RECORDS = os.path.join(ROOT, "test_records")      # side records of the checks (git-ignored)


def _env(**kw):
    return dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **kw)


def _verdict(path, log, rc):
    assert os.path.exists(path), "the worker wrote no verdict (exit %s):\n%s" % (rc, log[-3000:])
    v = json.load(open(path))
    os.makedirs(RECORDS, exist_ok=True)
    with open(os.path.join(RECORDS, "short_batch_%s.json" % os.path.basename(path)), "w") as f:
        json.dump(v, f, indent=1)
    failed = {k: c for k, c in v["checks"].items() if not c["ok"]}
    assert not failed and rc == 0 and v["ok"], (failed, log[-2000:])
    return v


@pytest.mark.parametrize("case,limit", [("oracle_bv5", 900), ("oracle_jhmdb_bv", 900), ("equal_large", 600), ("mixed", 600),
                                        ("stager", 600), ("refusal", 600)])
def test_short_step(tmp_path, case, limit):
    out = str(tmp_path / case)
    p = subprocess.run([sys.executable, WORKER, case, out], env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=limit)
    _verdict(out, p.stdout, p.returncode)


# the product engine (bs 8, 8 x 224 x 224) on every short size m = 3..7 against the oracle: labeled + unlabeled clips; UCF-101 for all five sizes
# (m = 5 both ways round), JHMDB for one odd m.  One process and time limit each.
ORACLE_224 = ["ucf_2+1", "ucf_2+2", "ucf_3+2", "ucf_1+4", "ucf_3+3", "ucf_4+3", "jhmdb_3+2"]


@pytest.mark.parametrize("tag", ORACLE_224)
def test_short_step_at_the_product_shape_vs_oracle(tmp_path, tag):
    """tests/short_batch_worker.py case_oracle224: scalars 1e-4, logits / masks 1e-3, check_gradients_fp64_anchored with its default floor,
    running statistics 1e-5 -- the bars of test_step_bs8_full_size_vs_oracle (4+3: a 2e-2 floor for one shown ReLU-mask flip, see the worker)."""
    case = "oracle224_" + tag
    out = str(tmp_path / case)
    p = subprocess.run([sys.executable, WORKER, case, out], env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    _verdict(out, p.stdout, p.returncode)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_full_and_short_step_on_one_gpu(tmp_path):
    """Rank 0 runs a full bs-4 step, rank 1 a (2 labeled, 1 unlabeled) step: both issue the same collectives in the same order (a
    mismatch would hang the group -- the time limit turns that into a failure), the reduced gradient is g_0 + g_1 bit for bit and both
    ranks hold the same parameters after Adam."""
    port = _free_port()
    out = str(tmp_path / "dp")
    procs = [subprocess.Popen([sys.executable, WORKER, "dp", out], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                              env=_env(RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for r in range(2):
        _verdict("%s.%d" % (out, r), logs[r], procs[r].returncode)


STANDIN = '''
"""Stand-in for the caller's datasets/ucf_dataloader.py: UCF101DataLoader items shaped as the reference's
(datasets/ucf_dataloader.py:179-191), synthetic content.  5 labeled, 7 unlabeled, 2 validation clips."""
import numpy as np
import torch
from torch.utils.data import Dataset


class UCF101DataLoader(Dataset):
    def __init__(self, name, clip_shape, file_id=None, use_random_start_frame=False):
        self.name, self.hw, self.file_id = name, clip_shape[0], file_id
        self.labeled = name != "train" or "unlabel" not in str(file_id)
        self.n = 2 if name != "train" else (5 if self.labeled else 7)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = np.random.default_rng(1000 * len(str(self.file_id)) + i)
        clip = torch.from_numpy(g.random((3, 8, self.hw, self.hw)))
        msk = torch.zeros(1, 8, self.hw, self.hw, dtype=torch.float64)
        y, x = int(g.integers(0, self.hw - 80)), int(g.integers(0, self.hw - 80))
        msk[:, :, y:y + 80, x:x + 80] = 1.0
        return {"data": clip, "loc_msk": msk, "action": torch.Tensor([int(g.integers(0, 24))]), "aug_data": torch.flip(clip, [3]),
                "label_vid": 1 if self.labeled else 0}
'''


@pytest.mark.parametrize("bs", [4, 5])
def test_dropin_epoch_over_the_callers_loaders(tmp_path, bs):
    """dropin/main_ucf101.py with PICONS_SYNTHETIC=0 over 5 labeled and 7 unlabeled clips: steps of 4, 4, 3 and 3 clips (the labeled
    loader restarts at the fourth), an engine built for 2 * (bs // 2) clips; the epoch ends, every loss is finite and a checkpoint is written."""
    ds = tmp_path / "datasets"
    ds.mkdir()
    (ds / "__init__.py").write_text("")
    (ds / "ucf_dataloader.py").write_text(textwrap.dedent(STANDIN))
    work = tmp_path / "run"
    work.mkdir()
    script = os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin", "main_ucf101.py")
    env = _env(PICONS_SYNTHETIC="0", PYTHONPATH=os.pathsep.join([str(tmp_path)] + [q for q in [os.environ.get("PYTHONPATH")] if q]))
    p = subprocess.run([sys.executable, script, "--bs", str(bs), "--epochs", "1", "--pf", "1", "--workers", "0", "--exp_id", "short"],
                       env=env, cwd=str(work), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    log = p.stdout
    assert p.returncode == 0, log[-3000:]
    lines = [ln for ln in log.splitlines() if ln.startswith("[TRAIN]")]
    assert len(lines) == 4, log[-3000:]
    for ln in lines:
        loss = float(ln.split("loss-")[1].split(",")[0])
        assert loss == loss and abs(loss) < 1e30, ln
    ckpts = [f for _d, _s, fs in os.walk(str(work / "train_log_wts" / "short")) for f in fs if f.endswith(".pth")]
    assert ckpts, log[-3000:]
