"""A numpy restatement of pc_frame_instances for the tests, written independently of the kernel's algorithm: a union-find over PIXELS (the kernel
labels row runs by propagating minima), components -> (area, box, first) -> rank -> imap.  Plus the row runs of a frame, counted on their
own, so that a test can assert which side of PC_INST_MAX_RUNS an input lies on."""
import numpy as np

HDR, WORDS, MAX_RUNS = 4, 6, 2048


def count_runs(frame):
    """Maximal horizontal foreground segments of one frame [H,W]."""
    fg = np.asarray(frame) != 0
    return int(fg[:, 0].sum() + (fg[:, 1:] & ~fg[:, :-1]).sum())


def components(frame, conn):
    """[H,W] -> [(area, x0, y0, x1, y1, first)] in the order of their first pixels (raster), by union-find over the foreground pixels."""
    fg = np.asarray(frame) != 0
    H, W = fg.shape
    parent = list(range(H * W))
    fgl = fg.tolist()

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    steps = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if conn == 8 else [])     # the neighbours that precede a pixel in raster order
    ys, xs = np.nonzero(fg)
    for y, x in zip(ys.tolist(), xs.tolist()):
        for dy, dx in steps:
            v, u = y + dy, x + dx
            if 0 <= v and 0 <= u < W and fgl[v][u]:
                a, b = find(y * W + x), find(v * W + u)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    comps = {}
    for y, x in zip(ys.tolist(), xs.tolist()):
        r = find(y * W + x)
        c = comps.get(r)
        if c is None:
            comps[r] = [1, x, y, x + 1, y + 1, y * W + x]
        else:
            c[0] += 1; c[1] = min(c[1], x); c[3] = max(c[3], x + 1); c[4] = max(c[4], y + 1)
    return [tuple(c) for c in sorted(comps.values(), key=lambda c: c[5])], parent, find


def frame_instances(frame, conn, min_area, K, max_runs=MAX_RUNS):
    """One frame -> (record int32 [4 + 6K], imap uint8 [H,W], n_runs)."""
    fg = np.asarray(frame) != 0
    H, W = fg.shape
    n_runs = count_runs(fg)
    rec = np.zeros(HDR + K * WORDS, np.int32)
    rec[2] = n_runs
    if n_runs > max_runs:
        rec[3] = 1
        return rec, np.where(fg, 255, 0).astype(np.uint8), n_runs
    comps, _parent, find = components(fg, conn)
    big = sorted((c for c in comps if c[0] >= min_area), key=lambda c: (-c[0], c[5]))
    rec[0], rec[1] = len(big), min(len(big), K)
    rank = {}
    for r, c in enumerate(big[:K]):
        rec[HDR + r * WORDS:HDR + (r + 1) * WORDS] = c
        rank[c[5]] = r + 1
    imap = np.zeros((H, W), np.uint8)
    for y, x in zip(*(a.tolist() for a in np.nonzero(fg))):
        imap[y, x] = rank.get(find(y * W + x), 255)          # a component's root is its first pixel: the smaller index wins every union
    return rec, imap, n_runs


def video_instances(mask, conn, min_area, K):
    """[F,H,W] -> (records int32 [F, 4 + 6K], imap uint8 [F,H,W], n_runs [F])."""
    out = [frame_instances(f, conn, min_area, K) for f in np.asarray(mask)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], np.int64)
