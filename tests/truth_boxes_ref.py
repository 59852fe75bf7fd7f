"""numpy restatement of pc_paint_boxes (include/picons.h): a rect table painted in table order, one assignment per rect.  What the device
entry (tests/test_truth_boxes_kernels_gpu.py) and evalstep.BoxTruth.dense (tests/test_truth_boxes_cpu.py) are held to."""
import numpy as np

MAX_RECTS, WORDS = 32, 5


def paint(rects, F, H, W, binary=False):
    """rects int [F, R, 5] of (x0, x1, y0, y1, value), half-open, each rect intersected with the frame -> uint8 [F, H, W]: a later rect
    overwrites an earlier one, a rect with x1 <= x0, y1 <= y0 or a zero low byte paints nothing; binary: 1 instead of the value."""
    rects = np.asarray(rects, np.int64)
    assert rects.shape[0] == F and rects.shape[2] == WORDS and 1 <= rects.shape[1] <= MAX_RECTS
    out = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for x0, x1, y0, y1, v in rects[f]:
            x0, x1, y0, y1 = max(int(x0), 0), min(int(x1), W), max(int(y0), 0), min(int(y1), H)
            v = int(v) & 255
            if x1 <= x0 or y1 <= y0 or v == 0:
                continue
            out[f, y0:y1, x0:x1] = 1 if binary else v
    return out
