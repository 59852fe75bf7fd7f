"""Overlapping clips in time restated in numpy float32, shared by tests/test_clip_hop_kernels_gpu.py and tests/test_clip_hop_gpu.py: which
clips hold a frame (the cover range of csrc/cliphop.h, from the text of include/picons.h), the merged logits of every clip
(tests/detectviews_ref.Merge, one clip at a time) and the mean over the windows that hold a frame, one float32 operation at a time in window
order: the first value as it is, the others added, one division by the count when it is above 1."""
import numpy as np

from tests.detectviews_ref import Merge


def ceil_div(a, b):
    return -(-a // b)


def cover_range(F, fs, hop, f):
    """-> (lo, hi): the windows that hold frame f of F."""
    span = 8 * fs
    windows = 1 if F <= span else 1 + ceil_div(F - span, hop)
    return max(0, ceil_div(f - span + 1, hop)), min(f // hop, windows - 1)


def holders(starts, F, fs, hop, f):
    """[(clip, frame of the clip)] of the clips that hold video frame f, in window order."""
    lo, hi = cover_range(F, fs, hop, f)
    out = []
    for m in range(lo, hi + 1):
        s = m * hop + f % fs
        out.append((starts.index(s), (f - s) // fs))
    return out


def restate(x, starts, F, fs, hop, views, Hs, Ws, S):
    """x float32 [V, n, 8, S, S], clip c cut at starts[c] -> (per clip merged logits float32 [n, 8, Hs, Ws], cover counts [Hs, Ws], the mean
    over the windows float32 [F, Hs, Ws])."""
    per, num = [], None
    for c in range(len(starts)):
        m = Merge(16, Hs, Ws, S)                                       # the clip as a video of its own: its frames at 0, 2, .., 14
        m.add(x[:, c:c + 1], views, [0])
        per.append(m.merged()[0::2].copy())
        assert num is None or np.array_equal(num, m.num[0])
        num = m.num[0].copy()
    mean = np.zeros((F, Hs, Ws), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            hold = holders(starts, F, fs, hop, f)
            acc = per[hold[0][0]][hold[0][1]].copy()
            for c, k in hold[1:]:
                acc = (acc + per[c][k]).astype(np.float32)
            mean[f] = (acc / np.float32(len(hold))).astype(np.float32) if len(hold) > 1 else acc
    return np.stack(per), num, mean
