#!/usr/bin/env python3
"""Diagnostic: per-tensor gradient error of one step against the fp64 oracle at an arbitrary batch / frame size (the check of
tests/test_step_gpu.py::check_gradients_fp64_anchored, printing every tensor that is clearly worse than the fp32 oracle).
    python tools/probe_bs_grads.py [bs] [hw] [stepid] [tensor names: their eight worst elements]
    python tools/probe_bs_grads.py <labeled>+<unlabeled> [hw] [bs] [tensor names]      a SHORT step of a bs-clip engine (default 8), the
                                                                                       configuration of tests/short_batch_worker.py
A ReLU-mask flip (a pre-activation within fp32 rounding of zero that lands on the other side in the fp64 run) shows as ONE channel of a
BatchNorm bias gradient -- a plain sum over positions -- carrying the tensor's whole error while the others agree to fp32 rounding."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import test_step_gpu as T

if len(sys.argv) > 1 and "+" in sys.argv[1]:
    from oracle import step as ostep
    from picons_amd import step as pstep, synthetic
    nl, nu = (int(v) for v in sys.argv[1].split("+"))
    hw = int(sys.argv[2]) if len(sys.argv) > 2 else 224
    bs = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    akw = dict(bv=True, n_frames=5, wt_cons=0.1)
    state = synthetic.init_state(47, 24)
    eng = pstep.StepEngine(pstep.default_args(lr=1e-4, **akw), bs=bs, hw=hw, num_classes=24, state=state)
    lab, unl, perm, drops = synthetic.make_step_inputs_split(nl, nu, num_classes=24, hw=hw)
    ramp = pstep.exp_rampup(100)(1)
    eng.stage(lab, unl, perm, drops)
    eng.forward_backward(1, ramp)
    eng.synchronize()
    oa = ostep.default_args(dataset="ucf101", **akw)
    P = ostep.as_torch_params(state)
    ostep.train_step(P, oa, lab, unl, 1, ramp, perm, drops)["total"].backward()
    P64 = ostep.as_torch_params(state, dtype=torch.float64)
    ostep.train_step(P64, oa, lab, unl, 1, ramp, perm, drops, dtype=torch.float64)["total"].backward()
    print("short step %d+%d on a bs-%d engine" % (nl, nu, bs))
else:
    bs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    hw = int(sys.argv[2]) if len(sys.argv) > 2 else 112
    stepid = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    eng, ref, P, P64 = T.run_pair(dict(bv=True, gv=True, n_frames=5, wt_cons=0.1), hw, bs, 1, 24, False, stepid=stepid)
rows = []
for name in eng.plan.pshape:
    g = eng.grad(name).cpu().double(); r32 = P[name].grad.double(); r64 = P64[name].grad
    den = r64.norm().item() + 1e-12
    rows.append((name, (g - r64).norm().item() / den, (r32 - r64).norm().item() / den, den))
print("bs %d hw %d lanes %s" % (bs, hw, os.environ.get("PICONS_LANES", "4")))
for r in rows:
    if r[1] > max(3 * r[2], 3e-3):
        print("%-44s hip %.3e  cpu32 %.3e  |g| %.3e" % r)

if len(sys.argv) > 4:
    for name in sys.argv[4:]:
        g = eng.grad(name).cpu().double().flatten(); r32 = P[name].grad.double().flatten(); r64 = P64[name].grad.flatten()
        d = (g - r64).abs(); d32 = (r32 - r64).abs()
        top = torch.argsort(d, descending=True)[:8]
        print(name, "n", g.numel(), "max|d| %.3e at %s; |r64| max %.3e" % (d.max().item(), top.tolist(), r64.abs().max().item()))
        print("   share of the squared error in the worst element: hip %.3f  cpu32 %.3f; without it rel-L2 hip %.3e" %
              ((d.max() ** 2 / (d ** 2).sum()).item(), (d32.max() ** 2 / (d32 ** 2).sum().clamp_min(1e-300)).item(),
               (((d ** 2).sum() - d.max() ** 2).clamp_min(0).sqrt() / r64.norm()).item()))
        for i in top.tolist():
            print("   [%d] hip %.6e  r32 %.6e  r64 %.6e   d %.2e  d32 %.2e" % (i, g[i], r32[i], r64[i], d[i], d32[i]))
