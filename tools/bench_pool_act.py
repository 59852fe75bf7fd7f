#!/usr/bin/env python3
"""The max-pool (forward / backward) and activation-backward launches of the bs = 8 training plan, one at a time on random data.

The shapes are read from the plan (its OP_POOL_FWD, OP_POOL_BWD and OP_ACT_BWD ops), not from a copied list.  Per launch: microseconds over
REPS launches between device events (after WARM warm ones), the footprint in MB -- every tensor the op has to touch counted once: input +
output + uint8 argmax forward; dy + argmax + dx (twice when it accumulates) backward; dy + y (+ dz) for the activation backward -- and the
footprint over the time in GB/s.  Run once per build of the library (PICONS_LIB_NAME) and compare; it is also the program to put behind
`rocprofv3 ... --` for counter and kernel-trace runs (REPS=1 WARM=0 then gives one launch per op, in the order printed).  ONLY=pool|act."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import picons_amd  # noqa
from picons_amd import capi, desc as D, ops, step as pstep
from picons_amd.plan import Plan

BS, HW = int(os.environ.get("BS", "8")), int(os.environ.get("HW", "224"))
REPS, WARM = int(os.environ.get("REPS", "20")), int(os.environ.get("WARM", "3"))
ONLY = os.environ.get("ONLY", "")
dev = "cuda"

plan = Plan(24, HW, n=BS, groups=2, training=True, lanes=4, early_adam=True)
plan.build_forward(); plan.build_loss(pstep.default_args(bv=True, n_frames=5)); plan.build_backward(); plan.build_adam()
plan.finalize()
g = torch.Generator(device=dev).manual_seed(1)


def rnd(*shape):
    return torch.randn(*shape, generator=g, device=dev)


def pool_desc(ints):
    d, q = {}, 0
    for f in D.POOL_FIELDS:
        n = 3 if f in ("k", "s", "padf") else 1
        d[f] = [int(v) for v in ints[q:q + 3]] if n == 3 else int(ints[q])
        q += n
    return d


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def pool_job(kind, ints):
    d = pool_desc(ints)
    npi, npo, C_ = d["N"] * d["Ti"] * d["Hi"] * d["Wi"], d["N"] * d["To"] * d["Ho"] * d["Wo"], d["C"]
    x, y = rnd(npi, d["ldi"]), rnd(npo, d["ldo"])
    am = torch.empty(npo, C_, device=dev, dtype=torch.uint8)
    name = "k%d%d%d s%d%d%d %dx%dx%dx%d" % (*d["k"], *d["s"], d["Ti"], d["Hi"], d["Wi"], C_)
    if kind == capi.OP_POOL_FWD:
        return "pool fwd " + name, 4 * C_ * (npi + npo) + npo * C_, lambda: ops.maxpool_fwd(d, x, y, am)
    am.copy_(torch.randint(0, d["k"][0] * d["k"][1] * d["k"][2], (npo, C_), generator=g, device=dev, dtype=torch.uint8))     # one winning tap per output
    acc = bool(ints[19])
    return "pool bwd " + name + (" +=" if acc else ""), 4 * C_ * (npo + npi * (2 if acc else 1)) + npo * C_, lambda: ops.maxpool_bwd(d, y, am, x, accum=acc)


def act_job(ints, longs, ptrs):
    lddy, ldy, act, C_, lddz, _acc = [int(v) for v in ints[:6]]
    rows = int(longs[0])
    dy = rnd(rows, lddy)
    yv = dy if ptrs[1] == ptrs[0] else torch.rand(rows, ldy, generator=g, device=dev)
    dz = None if ptrs[2] is None else (dy if ptrs[2] == ptrs[0] else torch.empty(rows, lddz, device=dev))
    db = None if ptrs[3] is None else torch.zeros(C_, device=dev)
    ws = torch.empty(int(capi.lib().pc_act_bwd_ws_floats(rows, C_)), device=dev)
    writes = dz is not None and (act != capi.ACT_NONE or dz is not dy)
    name = "act bwd %s %dx%d%s%s" % ({capi.ACT_NONE: "none", capi.ACT_RELU: "relu", capi.ACT_SIGMOID: "sigm"}[act], rows, C_,
                                     " dz" if writes else "", " dbias" if db is not None else "")
    nbytes = 4 * rows * C_ * ((1 if yv is dy or act == capi.ACT_NONE else 2) + (1 if writes else 0))

    def fn():
        capi.call("pc_act_bwd", ops.ptr(dy), lddy, ops.ptr(yv), ldy, act, C_, rows, ops.ptr(dz), lddz, ops.ptr(db), 0, ops.ptr(ws), ops.stream())
    return name, nbytes, fn


tot = {}
print("%-52s %9s %9s %9s" % ("launch", "us", "MB", "GB/s"))
for lst in ("fwd", "bwd"):
    for op in plan.lists[lst]:
        kind, ints, ptrs, longs = op[0], op[1], op[3], op[4]
        if kind in (capi.OP_POOL_FWD, capi.OP_POOL_BWD) and ONLY in ("", "pool"):
            fam = "pool fwd" if kind == capi.OP_POOL_FWD else "pool bwd"
            name, nbytes, fn = pool_job(kind, ints)
        elif kind == capi.OP_ACT_BWD and ONLY in ("", "act"):
            fam = "act bwd"
            name, nbytes, fn = act_job(ints, longs, ptrs)
        else:
            continue
        us = timed(fn)
        t = tot.setdefault(fam, [0.0, 0.0, 0])
        t[0] += us; t[1] += nbytes; t[2] += 1
        print("%-52s %9.1f %9.1f %9.0f" % (name, us, nbytes / 1e6, nbytes / us / 1e3), flush=True)
for fam, (us, nbytes, n) in tot.items():
    print("%-52s %9.1f %9.1f %9.0f" % ("sum %s (%d launches)" % (fam, n), us, nbytes / 1e6, nbytes / us / 1e3))
