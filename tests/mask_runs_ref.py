"""numpy restatement of pc_mask_run_index / pc_mask_runs, written from the contract in include/picons.h, not from the kernel: per row, the
positions where the byte value changes.  A run is a maximal horizontal segment of one non-zero value; rows are numbered over the given
frames, r = f * H + y; run words are (r | value << 24, x0 | x1 << 16) with x1 half-open."""
import numpy as np

RUN_WORDS = 2


def row_runs(row):
    """One row of bytes -> [(x0, x1, value)] from left to right."""
    row = np.asarray(row, np.uint8).reshape(-1)
    if row.size == 0:
        return []
    cuts = np.flatnonzero(row[1:] != row[:-1]) + 1                   # a new segment begins at every change of value
    x0s = np.concatenate([[0], cuts])
    x1s = np.concatenate([cuts, [row.size]])
    return [(int(a), int(b), int(row[a])) for a, b in zip(x0s, x1s) if row[a] != 0]


def runs_of(frames):
    """uint8 [nf, H, W] -> (index int32 [nf * H + 1], runs uint32 [n, 2]) as the two entries leave them for the range of these frames."""
    m = np.asarray(frames, np.uint8)
    nf, H, W = m.shape
    rows = m.reshape(nf * H, W)
    index = np.zeros(nf * H + 1, np.int64)
    words = []
    live = np.flatnonzero(rows.any(axis=1))                          # (a row of zeros has no runs: skipped for speed only)
    per_row = np.zeros(nf * H, np.int64)
    for r in live.tolist():
        rr = row_runs(rows[r])
        per_row[r] = len(rr)
        words.extend((r | v << 24, x0 | x1 << 16) for x0, x1, v in rr)
    index[1:] = np.cumsum(per_row)
    assert index[-1] < 2 ** 31
    return index.astype(np.int32), np.array(words, np.uint32).reshape(-1, RUN_WORDS)


def dense_of(runs, nf, H, W):
    """The inverse: run words -> uint8 [nf, H, W], painted run by run."""
    out = np.zeros((nf * H, W), np.uint8)
    for w0, w1 in np.asarray(runs, np.uint32).reshape(-1, RUN_WORDS).tolist():
        out[w0 & 0xffffff, (w1 & 0xffff):(w1 >> 16)] = w0 >> 24
    return out.reshape(nf, H, W)
