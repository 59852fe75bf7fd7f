"""GPU: pc_transpose_multi by job class, bit for bit.

One call of more than 40 jobs (more than one argument pack) mixes the three classes the entry point sorts its jobs into:
  C == 1 without slices -- dst[b][0][r] (+)= src[b][r][0], a copy per batch -- with R in {1, 3, 40}, batch in {1, 5}, a destination that
    starts 4 bytes off a 16-byte boundary, batch strides that are no multiple of 4 floats, and a source with src_ld > 1 (which is no copy);
  R == 1 -- dst[b][c][0] (+)= the sum over the K-slice images of src[b][0][c] -- with C in {4, 38, 40}, src_ld 40, 0 / 1 / 5 / 17 / 36
    slices, accum 0 and 1, dst_ld 1 and 3;
  everything else (the tile path): 27-tap and 2-D jobs, with and without slices.
The reference is float32 numpy: without slices the source element, with slices a sum from zero over the images in ascending order, then
(accum ? old : 0) + value -- single float32 additions in a fixed order, so the comparison is np.array_equal.  Sources carry signed zeros.
Every destination buffer is prefilled (canary, or the old values where the job accumulates), the words a job does not own must keep the
canary, and the call runs twice to equal bits."""
import numpy as np
import pytest
import torch

from picons_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = np.float32(-777.25)


def _job(rng, batch, R, C, sld=None, dld=None, nsl=0, accum=0, dst_off=0, sbs_pad=0, dbs_pad=0):
    """-> dict with the host source / old destination, the strides and the expected destination buffer"""
    sld = C if sld is None else sld
    dld = R if dld is None else dld
    sbs = R * sld + sbs_pad
    dbs = C * dld + dbs_pad
    nim = max(nsl, 1)
    sst = -(-(batch * sbs) // 4) * 4 + 8                 # floats between two slice images, a multiple of 4
    src = rng.standard_normal(nim * sst + 4).astype(np.float32)
    src[rng.random(src.shape) < 0.1] = np.float32(-0.0)   # 0 + (-0) is +0: the `0 +` of the expression is visible
    src[rng.random(src.shape) < 0.05] = np.float32(0.0)
    dst = np.full(dst_off + batch * dbs + 5, CANARY, dtype=np.float32)
    old = rng.standard_normal(dst.shape).astype(np.float32)
    old[rng.random(old.shape) < 0.1] = np.float32(-0.0)
    want = dst.copy()
    for b in range(batch):
        for r in range(R):
            for c in range(C):
                if nsl <= 1:
                    v = src[b * sbs + r * sld + c]
                else:
                    v = np.float32(0.0)
                    for k in range(nsl):
                        v = np.float32(v + src[k * sst + b * sbs + r * sld + c])
                at = dst_off + b * dbs + c * dld + r
                want[at] = np.float32((old[at] if accum else np.float32(0.0)) + v)
    if accum:
        own = want != CANARY
        dst[own] = old[own]
    return dict(src=src, dst0=dst, want=want, args=(batch, R, C, sbs, sld, dbs, dld, accum, nsl, sst), dst_off=dst_off)


def _jobs():
    rng = np.random.default_rng(7)
    J = []
    # C == 1 without slices: copies
    for R in (1, 3, 40):
        for batch in (1, 5):
            for accum in (0, 1):
                J.append(_job(rng, batch, R, 1, accum=accum))
    J.append(_job(rng, 5, 40, 1, dst_off=1))                       # destination 4 bytes off a 16-byte boundary
    J.append(_job(rng, 5, 40, 1, dst_off=1, accum=1))
    J.append(_job(rng, 5, 40, 1, sbs_pad=2, dbs_pad=3))            # batch rows that do not start on 16-byte boundaries
    J.append(_job(rng, 1, 1100, 1, accum=1))                       # more than one block of quads
    J.append(_job(rng, 5, 3, 1, sld=2, dld=4))                     # C == 1 read with a stride: no copy, the tile path
    # R == 1 with slices (src_ld 40), and without
    for C in (4, 38, 40):
        for nsl in (0, 1, 5, 17, 36):
            for accum in (0, 1):
                J.append(_job(rng, 3, 1, C, sld=40, dld=1, nsl=nsl, accum=accum))
    J.append(_job(rng, 2, 1, 38, sld=40, dld=3, nsl=17, accum=1))   # destination elements dst_ld = 3 apart
    J.append(_job(rng, 2, 1, 38, sld=40, dld=3, nsl=0, accum=0))
    J.append(_job(rng, 7, 1, 300, sld=300, dld=1, nsl=36, accum=0, dst_off=2))     # more than one block; unaligned destination
    J.append(_job(rng, 1, 1, 37, sld=37, dld=1, nsl=0, accum=1))    # no slices, an odd row: 4-byte loads
    # the tile path: 27 taps, 2-D, with and without slices
    J.append(_job(rng, 4, 6, 27, dld=6))
    J.append(_job(rng, 4, 27, 6, accum=1))
    J.append(_job(rng, 1, 45, 70))
    J.append(_job(rng, 2, 27, 38, sld=40, nsl=5, accum=1))
    J.append(_job(rng, 1, 33, 36, sld=36, nsl=17))
    rows = sum(1 for j in J if j["args"][1] == 1 or (j["args"][2] == 1 and j["args"][4] == 1 and j["args"][8] <= 1))
    assert rows >= 41 and len(J) - rows >= 5                        # the row jobs alone cross an argument pack of 40
    order = rng.permutation(len(J))                                 # the classes mixed
    return [J[q] for q in order]


def test_transpose_multi_by_class():
    J = _jobs()
    srcs = [torch.from_numpy(j["src"]).to(DEV) for j in J]
    assert all(s.data_ptr() % 16 == 0 for s in srcs)
    runs = []
    for _ in range(2):
        dsts = [torch.from_numpy(j["dst0"]).to(DEV) for j in J]
        assert all(d.data_ptr() % 16 == 0 for d in dsts)
        jobs = []
        for j, s, d in zip(J, srcs, dsts):
            batch, R, C, sbs, sld, dbs, dld, accum, nsl, sst = j["args"]
            jobs.append((s, d[j["dst_off"]:], batch, R, C, sbs, sld, dbs, dld, accum, nsl, sst))
        ops.transpose_multi(jobs)
        torch.cuda.synchronize()
        runs.append([d.cpu().numpy() for d in dsts])
    for q, j in enumerate(J):
        a, b = runs[0][q], runs[1][q]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "job %d %r: two runs differ" % (q, j["args"])
        assert np.array_equal(a.view(np.uint32), j["want"].view(np.uint32)), "job %d %r" % (q, j["args"])
    for j, s in zip(J, srcs):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), j["src"].view(np.uint32)), "a source was written"
