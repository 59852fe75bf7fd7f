"""numpy restatement of pc_prob_truth_hist (csrc/probhist.hip), written from its contract in include/picons.h: every pixel's (truth or not,
number of threshold words at or below its probability word) pair added into its frame's table with np.add.at; and of detect.sweep_counts from
the definition of a mask threshold.  The yardstick of tests/test_detect_sweep_cpu.py and the two GPU test files: exact to the integer."""
import numpy as np


def hist(prob, truth, words):
    """prob uint16 [F, H, W], truth uint8 [F, H, W], words ascending -> int32 [F, 2, N + 1]: table[f, t, b] the pixels of frame f with truth
    zero (t = 0) or not (t = 1) and exactly b words <= the pixel's probability word."""
    prob, truth = np.asarray(prob), np.asarray(truth)
    assert prob.dtype == np.uint16 and truth.dtype == np.uint8 and prob.ndim == 3 and prob.shape == truth.shape
    w = np.asarray(words).astype(np.int64).reshape(-1)
    assert w.size >= 1 and w[0] >= 1 and w[-1] <= 65535 and (np.diff(w) > 0).all()
    F = prob.shape[0]
    out = np.zeros((F, 2, w.size + 1), np.int32)
    f = np.broadcast_to(np.arange(F)[:, None, None], prob.shape)
    b = np.searchsorted(w, prob.astype(np.int64), side="right")
    np.add.at(out, (f.reshape(-1), (truth != 0).astype(np.int64).reshape(-1), b.reshape(-1)), 1)
    return out


def sweep_counts(table):
    """int32 [F, 2, N + 1] -> int64 [N, F, 3]: (inter, union, gt) of the mask `more than k words at or below the pixel`, one k at a time."""
    t = np.asarray(table).astype(np.int64)
    F, N = t.shape[0], t.shape[2] - 1
    out = np.zeros((N, F, 3), np.int64)
    for k in range(N):
        for f in range(F):
            inter, gt = t[f, 1, k + 1:].sum(), t[f, 1, :].sum()
            out[k, f] = (inter, gt + t[f, 0, k + 1:].sum(), gt)
    return out


def brute_counts(prob, truth, words):
    """The definition, threshold by threshold: the mask q >= word against truth != 0 -> int64 [N, F, 3] = (inter, union, gt)."""
    prob, g = np.asarray(prob), np.asarray(truth) != 0
    F = prob.shape[0]
    out = np.zeros((len(words), F, 3), np.int64)
    for k, w in enumerate(words):
        m = prob >= int(w)
        out[k, :, 0] = (m & g).reshape(F, -1).sum(1)
        out[k, :, 1] = (m | g).reshape(F, -1).sum(1)
        out[k, :, 2] = g.reshape(F, -1).sum(1)
    return out
