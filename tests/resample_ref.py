"""pc_resample_tables and the bilinear way back of pc_detect_frames_scaled restated in numpy float32 from the text of include/picons.h, shared
by tests/test_detect_scaled_cpu.py, test_detect_scaled_kernels_gpu.py and test_detect_scaled_gpu.py.  It sits on top of
tests/detectviews_ref.Merge, which reproduces the merged logit and the cover count of a working pixel bit for bit.

The table index is exact integer arithmetic: axis_pair states it in Python integers for one destination index, axis_table for a whole axis
in int64 (|num| < 2^56 for every size the library takes; the CPU test holds the two to each other).  The bilinear rule is written with
float32 arrays one operation at a time -- numpy rounds every float32 product and sum to nearest and fuses nothing, as __fmul_rn / __fadd_rn
do -- and a tap of zero weight is not read: np.where drops it, so a NaN under it poisons nothing."""
import numpy as np
import torch

from tests.detectviews_ref import Merge, box_of, real_frames, score_refs  # noqa: F401  (the tests build on them)


def axis_pair(L, D, d):
    """Destination index d of D from a source of length L -> (i0, r, den) in Python integers: w1 = float32(r) / float32(den)."""
    num, den = (2 * d + 1) * L - D, 2 * D
    i0 = num // den                                                   # floor
    r = num - i0 * den
    if i0 < 0:
        i0, r = 0, 0
    if i0 >= L - 1:
        i0, r = L - 1, 0
    return i0, r, den


def axis_table(L, D):
    """-> (i0 int64 [D], w1 float32 [D]) of a whole axis."""
    assert L >= 1 and D >= 1 and 2 * D < 1 << 24
    d = np.arange(D, dtype=np.int64)
    den = np.int64(2 * D)
    num = (2 * d + 1) * np.int64(L) - np.int64(D)
    i0 = np.floor_divide(num, den)
    r = num - i0 * den
    lo, hi = i0 < 0, i0 >= L - 1
    i0 = np.where(lo, 0, np.where(hi, L - 1, i0))
    r = np.where(lo | hi, 0, r)
    w1 = r.astype(np.float32) / np.float32(den)                       # both exact in float32: one rounding
    return i0, w1.astype(np.float32)


def tables(Hs, Ws, H, W):
    """The int32 words pc_resample_tables writes: rows [H][2], then columns [W][2], each pair (i0, bits of float32 w1)."""
    out = np.empty(2 * (H + W), np.int32)
    for o, (L, D) in ((0, (Hs, H)), (2 * H, (Ws, W))):
        i0, w1 = axis_table(L, D)
        out[o:o + 2 * D:2] = i0
        out[o + 1:o + 2 * D:2] = w1.view(np.int32)
    return out


def resample(M, num, H, W):
    """M float32 [..., Hs, Ws] merged logits, num [..., Hs, Ws] cover counts -> (v float32 [..., H, W], covered bool [..., H, W])."""
    M = np.asarray(M, np.float32)
    cov = np.asarray(num) >= 1
    Hs, Ws = M.shape[-2:]
    iy, wy1 = axis_table(Hs, H)
    ix, wx1 = axis_table(Ws, W)
    one = np.float32(1.0)
    wy0, wx0 = (one - wy1).astype(np.float32), (one - wx1).astype(np.float32)
    iy1, ix1 = np.minimum(iy + 1, Hs - 1), np.minimum(ix + 1, Ws - 1)       # read only under a non-zero weight, where they are iy + 1, ix + 1
    zx, zy = wx1 == 0, (wy1 == 0)[:, None]

    def row(r):
        a, b = M[..., r, :][..., ix], M[..., r, :][..., ix1]
        with np.errstate(invalid="ignore", over="ignore"):
            mixed = ((a * wx0).astype(np.float32) + (b * wx1).astype(np.float32)).astype(np.float32)
        ca, cb = cov[..., r, :][..., ix], cov[..., r, :][..., ix1]
        return np.where(zx, a, mixed), ca & (cb | zx)

    top, ctop = row(iy)
    bot, cbot = row(iy1)
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = ((top * wy0[:, None]).astype(np.float32) + (bot * wy1[:, None]).astype(np.float32)).astype(np.float32)
    return np.where(zy, top, mixed).astype(np.float32), ctop & (cbot | zy)


def masks(v, covered):
    """uint8: the evaluator's predicate as the reference states it (fp32 sigmoid(x) >= 0.5 on the host) on the covered pixels."""
    pos = (torch.sigmoid(torch.from_numpy(np.ascontiguousarray(v, np.float32))) >= 0.5).numpy()
    return (pos & covered).astype(np.uint8)


def expected_probs(v, covered):
    """GPU only.  pc_frame_probs' conversion of restated native logits v float32 [F, H, W] -> uint16 [F, H, W]: the existing entry run on
    them, the frames laid out as the clips of one uncropped view of a square frame at f_skip = 1.  An uncovered pixel enters as NaN, which
    the conversion takes to 0 as it takes a NaN logit.  (include/picons.h defines the scaled entry's map as that conversion of v; float32
    expf is the device's, which no host restatement reproduces bit for bit.)"""
    from picons_amd import ops
    F, H, W = v.shape
    S2 = (max(H, W) + 3) // 4 * 4
    n = (F + 7) // 8
    x = torch.zeros(n, 8, S2, S2, device="cuda")
    x.view(n * 8, S2, S2)[:F, :H, :W] = torch.from_numpy(np.where(covered, v, np.float32(np.nan)).astype(np.float32)).cuda()
    out = ops.frame_probs(x, [(0, 0, 0)], list(range(0, F, 8)), F, S2, S2, f_skip=1)
    return out.cpu().numpy().view(np.uint16)[:, :H, :W].copy()
