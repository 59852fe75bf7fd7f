"""pc_instance_overlaps restated in numpy, shared by tests/test_instance_links_cpu.py, test_instance_links_kernels_gpu.py and
test_instance_links_gpu.py.  Written from the entry's description in include/picons.h, not from the kernel: the slot of every pixel from its
map value, then per (frame, lag) one 2-D histogram over the pixels that are non-zero in both frames.  Integers throughout: exact."""
import numpy as np

MAX_LAGS = 4


def slots(imap, K):
    """Map values uint8 (any shape) -> int64 slots: r for the value r + 1 <= K, K for every other non-zero value, -1 for 0."""
    v = np.asarray(imap).astype(np.int64)
    return np.where(v == 0, -1, np.where(v <= K, v - 1, K))


def overlaps(imap, K, L):
    """imap uint8 [F,H,W] -> int32 [F, L, K + 1, K + 1]: [f, l, a, b] the pixels of slot a in frame f and of slot b in frame f + l + 1; a lag
    whose later frame does not exist stays zero."""
    imap = np.asarray(imap)
    assert imap.dtype == np.uint8 and imap.ndim == 3 and 1 <= K <= 32 and 1 <= L <= MAX_LAGS
    F = imap.shape[0]
    s = slots(imap, K).reshape(F, -1)
    out = np.zeros((F, L, K + 1, K + 1), np.int64)
    for f in range(F):
        for lag in range(L):
            g = f + lag + 1
            if g >= F:
                continue
            both = (s[f] >= 0) & (s[g] >= 0)
            out[f, lag] = np.bincount(s[f][both] * (K + 1) + s[g][both], minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    assert out.max(initial=0) < 2 ** 31
    return out.astype(np.int32)


def slot_pixels(imap, K):
    """imap uint8 [F,H,W] -> int64 [F, K + 1]: the pixels of every slot."""
    F = np.asarray(imap).shape[0]
    s = slots(imap, K).reshape(F, -1)
    return np.stack([np.bincount(r[r >= 0], minlength=K + 1) for r in s])


def instance_fields(imap, K):
    """What a test needs of a frame's instances to link them, from a map whose values are ranks + 1 already: kept [F], boxes [F,K,4]
    (x0, y0, x1, y1, half-open), areas [F,K]."""
    imap = np.asarray(imap)
    F = imap.shape[0]
    kept, boxes, areas = np.zeros(F, np.int32), np.zeros((F, K, 4), np.int32), np.zeros((F, K), np.int32)
    for f in range(F):
        for r in range(K):
            ys, xs = np.nonzero(imap[f] == r + 1)
            if ys.size:
                assert kept[f] == r, "ranks of a frame are 0 .. kept - 1 without a hole"
                kept[f] = r + 1
                areas[f, r] = ys.size
                boxes[f, r] = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
    return kept, boxes, areas
