"""numpy restatement of pc_map_crosstab (csrc/crosstab.hip), written from its contract in include/picons.h: every pixel's (pred slot, truth
slot) pair added into its frame's table with np.add.at.  The yardstick of tests/test_detect_score_cpu.py and the two GPU test files: exact to
the integer."""
import numpy as np


def slots(values, n):
    """Byte values -> slots: 0 stays 0, 1..n keep their value, everything above n is n + 1."""
    v = np.asarray(values).astype(np.int64)
    return np.where(v <= n, v, n + 1)


def crosstab(pred, truth, P, A):
    """pred, truth uint8 [F, H, W] -> int32 [F, P + 2, A + 2]: table[f, p, a] the pixels of frame f with pred slot p and truth slot a."""
    pred, truth = np.asarray(pred), np.asarray(truth)
    assert pred.dtype == np.uint8 and truth.dtype == np.uint8 and pred.ndim == 3 and pred.shape == truth.shape
    F = pred.shape[0]
    out = np.zeros((F, P + 2, A + 2), np.int32)
    f = np.broadcast_to(np.arange(F)[:, None, None], pred.shape)
    np.add.at(out, (f.reshape(-1), slots(pred, P).reshape(-1), slots(truth, A).reshape(-1)), 1)
    return out


def seg_counts(pred01, truth):
    """The definition of pc_seg_frame_counts (csrc/evalmetrics.hip) for a 0 / 1 prediction: per frame #(pred + gt == 2), #(pred + gt != 0),
    #(gt != 0) -> int64 [F, 3]."""
    p, g = np.asarray(pred01).astype(np.float32), np.asarray(truth).astype(np.float32)
    v = (p + g).reshape(p.shape[0], -1)
    return np.stack([(v == 2).sum(1), (v != 0).sum(1), (g.reshape(p.shape[0], -1) != 0).sum(1)], axis=1).astype(np.int64)
