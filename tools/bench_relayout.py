#!/usr/bin/env python3
"""The weight re-layouts (pc_transpose_multi) and the tail scatter (pc_tail6_scatter) of the bs = 8 training plan, on random data.

The jobs are read from the plan -- every OP_TRANSPOSE of its lists and every job of its OP_TRANSPOSE_MULTI ops, and the arguments of its
OP_TAIL6_SCATTER -- not from a copied list.  The transpose jobs are sorted into the classes pc_transpose_multi sorts them into (C == 1
read with unit stride and without slices: a copy per batch; R == 1: a row, summed over its K-slice images; everything else: tiles), and
each class runs as ONE call on buffers of its own.  Per class and for the scatter: microseconds over REPS calls between device events
(after WARM warm ones), the footprint in MB -- every source image and every destination counted once, a destination twice when the job
accumulates; dout + dcols for the scatter -- and the footprint over the time in GB/s.  Run once per build of the library
(PICONS_LIB_NAME) and compare; it is also the program to put behind `rocprofv3 --kernel-trace ... --` (REPS=1 WARM=0: one call per
class, in the order printed).  ONLY=transpose|scatter."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import picons_amd  # noqa
from picons_amd import capi, ops, step as pstep
from picons_amd.plan import Plan

BS, HW = int(os.environ.get("BS", "8")), int(os.environ.get("HW", "224"))
REPS, WARM = int(os.environ.get("REPS", "20")), int(os.environ.get("WARM", "3"))
ONLY = os.environ.get("ONLY", "")
dev = "cuda"

plan = Plan(24, HW, n=BS, groups=2, training=True, lanes=4, early_adam=True)
plan.build_forward(); plan.build_loss(pstep.default_args(bv=True, n_frames=5)); plan.build_backward(); plan.build_adam()
plan.finalize()
g = torch.Generator(device=dev).manual_seed(1)


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


def plan_jobs():
    """(ints, longs) of every transpose job of the step"""
    jobs = []
    for lst in plan.lists.values():
        for op in lst:
            if op[0] == capi.OP_TRANSPOSE:
                jobs.append((op[1], op[4]))
            elif op[0] == capi.OP_TRANSPOSE_MULTI and op[3] and op[3][0][0] == "JOBS":
                jobs.extend((j[1], j[4]) for j in plan.multi_jobs[op[3][0][1]])
    return jobs


def job_class(i):
    batch, R, C, sld = i[:4]
    nsl = i[6] if len(i) > 6 else 0
    if R == 1:
        return "R == 1 (rows, slices summed)"
    if C == 1 and sld == 1 and nsl <= 1:
        return "C == 1 (copies)"
    return "tiles"


def make_job(i, l):
    batch, R, C, sld, dld, accum = [int(v) for v in i[:6]]
    nsl, sst = (int(i[6]), int(l[2])) if len(i) > 6 else (0, 0)
    sbs, dbs = int(l[0]), int(l[1])
    nim = max(nsl, 1)
    src = torch.randn((nim - 1) * sst + (batch - 1) * sbs + (R - 1) * sld + C + 4, generator=g, device=dev)
    dst = torch.zeros((batch - 1) * dbs + (C - 1) * dld + R, device=dev)
    nbytes = 4 * batch * R * C * (nim + (2 if accum else 1))
    return (src, dst, batch, R, C, sbs, sld, dbs, dld, accum, nsl, sst), nbytes


print("%-44s %6s %9s %9s %9s" % ("class", "jobs", "us", "MB", "GB/s"))
if ONLY in ("", "transpose"):
    classes = {}
    for i, l in plan_jobs():
        classes.setdefault(job_class(i), []).append((i, l))
    tot_us = tot_b = 0.0
    for name in sorted(classes):
        made = [make_job(i, l) for i, l in classes[name]]
        jobs, nbytes = [m[0] for m in made], sum(m[1] for m in made)
        us = timed(lambda: ops.transpose_multi(jobs))
        tot_us += us; tot_b += nbytes
        print("%-44s %6d %9.1f %9.1f %9.0f" % ("transpose " + name, len(jobs), us, nbytes / 1e6, nbytes / us / 1e3), flush=True)
        del made, jobs
    print("%-44s %6d %9.1f %9.1f %9.0f" % ("sum transposes", sum(len(v) for v in classes.values()), tot_us, tot_b / 1e6, tot_b / tot_us / 1e3))
if ONLY in ("", "scatter"):
    for lst in plan.lists.values():
        for op in lst:
            if op[0] != capi.OP_TAIL6_SCATTER:
                continue
            N, It, Ih, Iw = [int(v) for v in op[1][:4]]
            dout = torch.randn(N, 2 * It, 2 * Ih, 2 * Iw, generator=g, device=dev)
            dcols = torch.empty(N, It, Ih, Iw, 128, device=dev)
            nbytes = 4 * (dout.numel() + dcols.numel())
            us = timed(lambda: ops.tail6_scatter(dout, N, It, Ih, Iw, dcols))
            print("%-44s %6d %9.1f %9.1f %9.0f" % ("tail6 scatter %dx%dx%dx%d" % (N, It, Ih, Iw), 1, us, nbytes / 1e6, nbytes / us / 1e3), flush=True)
