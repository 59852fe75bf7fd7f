"""numpy restatement of pc_prob_cut (csrc/probcut.hip), written from its contract in include/picons.h: the mask q >= word, and per frame the
count of positive pixels, their half-open box from np.nonzero, and the score np.float32(np.float64(S) / (65535.0 * c)) with S the integer sum
of the probability words of the positive pixels."""
import numpy as np

ONE = 65535


def cut(prob, word):
    """prob np.uint16 [F,H,W], word in 1..65535 -> (mask uint8 [F,H,W], words int32 [F,6]: count, x0, y0, x1, y1, float32 score bits)."""
    prob = np.asarray(prob)
    assert prob.dtype == np.uint16 and prob.ndim == 3 and 1 <= int(word) <= ONE
    mask = (prob >= np.uint16(word)).astype(np.uint8)
    out = np.zeros((prob.shape[0], 6), np.int32)
    for f in range(prob.shape[0]):
        ys, xs = np.nonzero(mask[f])
        c = int(ys.size)
        if c == 0:
            continue                                          # count 0, box zeros, the bits of 0.0f
        S = int(prob[f][mask[f] != 0].astype(np.int64).sum())
        score = np.float32(np.float64(S) / (65535.0 * c))
        out[f] = [c, xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, int(np.array([score], np.float32).view(np.int32)[0])]
    return mask, out
