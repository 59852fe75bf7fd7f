#!/usr/bin/env python3
"""Host cost of a training-state checkpoint at full size (224 px, 24 classes: P, M, V of plan.nparams floats plus the running statistics):
the time to write one (StepEngine.train_state + trainstate.save: drain the engine, three device-to-host copies, torch.save, os.replace),
the time to load one (trainstate.load + StepEngine.load_train_state, which ends synchronised), the file's size, and beside them an epoch
of the synthetic run the write sits in (--steps train steps on fresh synthetic minibatches, then the engine drained).  Host clocks around
calls that end synchronised; medians of --runs runs, every single time listed.

    python tools/bench_trainstate.py [--bs 8] [--steps 4] [--runs 5] [--dir DIR] [--out profiles/trainstate_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import picons_amd  # noqa: F401,E402
from picons_amd import step as pstep, synthetic, trainstate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--steps", type=int, default=4, help="steps of the epoch the write is compared with (the drop-in's PICONS_STEPS default)")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory the state file is written to (default: a temporary one)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_trainstate.py measures on a GPU; there is none here")
    args = pstep.default_args(bv=True, n_frames=5, wt_cons=0.1, lr=1e-4, epochs=100)
    eng = pstep.StepEngine(args, bs=a.bs, hw=a.hw)
    ramp = pstep.exp_rampup(100)(1)

    def epoch():
        for i in range(a.steps):
            lab, unl, perm, drops = synthetic.make_step_inputs(a.bs, step=i, hw=a.hw)
            eng.train_step(lab, unl, 1, ramp, perm, drops)
        eng.synchronize()

    def full_state():
        ts = eng.train_state()
        return {"format": trainstate.FORMAT, "version": trainstate.VERSION, "model": ts["model"], "optimizer": ts["optimizer"],
                "scheduler": {}, "epoch": 1, "best": {}, "rng": trainstate.rng_state(), "args": dict(vars(args)),
                "meta": dict(num_classes=24, hw=a.hw, dataset="ucf101", world=1, fused=True)}

    epoch()                                    # warm-up: plans built, moments non-zero
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        path = os.path.join(d, "train_state.pt")
        t_epoch, t_write, t_load = [], [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            epoch()
            t1 = time.perf_counter()
            trainstate.save(path, full_state())
            t2 = time.perf_counter()
            eng.load_train_state(trainstate.load(path))
            t3 = time.perf_counter()
            t_epoch.append(t1 - t0); t_write.append(t2 - t1); t_load.append(t3 - t2)
        size = os.path.getsize(path)
    med = statistics.median
    res = dict(bs=a.bs, hw=a.hw, steps=a.steps, runs=a.runs, nparams=eng.plan.nparams, nrunning=eng.plan.nrunning, file_bytes=size,
               write_s=t_write, load_s=t_load, epoch_s=t_epoch, write_median_s=med(t_write), load_median_s=med(t_load),
               epoch_median_s=med(t_epoch), write_over_epoch=med(t_write) / med(t_epoch))
    print(json.dumps(res))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
