"""pc_wino_weights_multi: the Winograd weight transforms of many layers in one launch (the planner merges the per-step transforms of
every prep lane into it).  Each job runs the instructions of the single launch it replaces, so the bar is bit-equality with
pc_wino_weights / pc_wino4_weights -- including the zero padding of the last 64-channel block."""
import pytest
import torch

from picons_amd import capi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_three_jobs_equal_three_single_launches():
    g = torch.Generator().manual_seed(3)
    # (O, I, flip, m) over master OIDHW weights w[co][ci][3][3][3]: F(2x2) forward with 32 output channels (half a 64-channel block is
    # zero padding) from 64; F(2x2) input gradient (O / I exchanged: transposed strides, mirrored taps) 64 from 32; F(4x4) forward 64 from 64
    cases = [(32, 64, False, 2), (64, 32, True, 2), (64, 64, False, 4)]
    jobs, singles = [], []
    for O, I, flip, m in cases:
        co, ci = (I, O) if flip else (O, I)
        w = torch.randn(co, ci, 3, 3, 3, generator=g).to(DEV)
        strides = (27, 1, ci * 27) if flip else (ci * 27, 1, 27)
        n = int((capi.lib().pc_wino4_u_floats if m == 4 else capi.lib().pc_wino_u_floats)(O, I, 3))
        U = torch.full((n,), float("nan"), device=DEV)
        jobs.append((w, U, strides, O, I, 3, flip, m))
        singles.append(ops.wino_weights(w, O, I, 3, flip=flip, strides=strides, m=m))
    ops.wino_weights_multi(jobs)
    for (O, I, flip, m), job, ref in zip(cases, jobs, singles):
        assert job[1].numel() == ref.numel() and torch.isfinite(ref).all()
        assert torch.equal(job[1], ref), "job O=%d I=%d flip=%d m=%d: %d of %d elements differ" % (O, I, flip, m, (job[1] != ref).sum().item(), ref.numel())


def test_multi_refuses_a_bad_job():
    w = torch.zeros(64 * 64 * 27, device=DEV)
    with pytest.raises(RuntimeError, match="bad job 1"):
        ops.wino_weights_multi([(w, w, (64 * 27, 1, 27), 64, 64, 3, False, 2), (w, w, (27, 1, 27), 64, 12, 3, False, 2)])
