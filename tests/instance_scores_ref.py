"""pc_frame_probs and pc_instance_scores restated in numpy, shared by tests/test_instance_scores_cpu.py, test_instance_scores_kernels_gpu.py
and test_instance_scores_gpu.py.  The merged logits come from tests/detectviews_ref.Merge, which reproduces the kernels' merge bit for bit;
the probability is taken in float64 and left unrounded, so that a test states its own distance to it; the per-slot sums are integers and
exact."""
import numpy as np
import torch

from tests.detectviews_ref import Merge  # noqa: F401  (the tests build their merged logits with it)

ONE, WORDS = 65535, 3


def sigmoid64(m):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(m, np.float64)))


def q_exact(merged, num):
    """float64 65535 * sigmoid(m) per pixel, unrounded; 0 where no view covers the pixel (num == 0) or m is a NaN."""
    q = ONE * sigmoid64(merged)
    return np.where((np.asarray(num) > 0) & ~np.isnan(merged), q, 0.0)


def q_bound(merged):
    """How far the kernel's uint16 may lie from q_exact: 0.5 for the rounding to an integer, 2^-8 for the spacing of the fp32 product below
    65536 (half an ulp of 2^-8 twice: the product's own rounding and its argument's), and the fp32 sigmoid's distance from float64 carried to
    LSBs by the rule the frame scores are held to (tests/test_detect_views_kernels_gpu.py): the larger of 1e-6 and twice the distance of an
    fp32 torch evaluation."""
    m32 = torch.from_numpy(np.ascontiguousarray(merged, np.float32))
    s32 = (1.0 / (1.0 + torch.exp(-m32))).numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        d32 = np.nan_to_num(np.abs(s32 - sigmoid64(merged)), nan=0.0)
    return 0.5 + 2.0 ** -8 + ONE * np.maximum(1e-6, 2.0 * d32)


def slot_sums(imap, prob, K):
    """imap uint8 [F,H,W], prob uint16 [F,H,W] -> (sums int64 [F, K + 1], npix int64 [F, K + 1]): slot r < K the pixels with map value r + 1,
    slot K every other non-zero value."""
    imap, prob = np.asarray(imap), np.asarray(prob)
    assert imap.dtype == np.uint8 and prob.dtype == np.uint16 and imap.shape == prob.shape
    F = imap.shape[0]
    sums, npix = np.zeros((F, K + 1), np.int64), np.zeros((F, K + 1), np.int64)
    for f in range(F):
        v = imap[f].reshape(-1).astype(np.int64)
        slot = np.where(v <= K, v - 1, K)[v > 0]
        q = prob[f].reshape(-1).astype(np.int64)[v > 0]
        sums[f] = [q[slot == j].sum() for j in range(K + 1)]
        npix[f] = np.bincount(slot, minlength=K + 1)
    return sums, npix


def words(sums, npix):
    """The int32 record [F, 3 * (K + 1)] the kernel writes for these sums and counts."""
    sums = np.asarray(sums, np.int64)
    out = np.stack([sums & 0xffffffff, sums >> 32, np.asarray(npix, np.int64)], axis=2).astype(np.uint32).view(np.int32)
    return out.reshape(sums.shape[0], -1)
