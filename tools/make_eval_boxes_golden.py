#!/usr/bin/env python3
"""AUTHORING CONTAINER ONLY: run the reference's own evaluation loader `UCF101DataLoader.load_video` (datasets/ucf_dataloader_eval.py:110-160)
on tiny synthetic videos and record, per case, the annotations it was given, the np.random seed, and the `bbox` array it returned, in
tests/golden/eval_boxes.npz.  Stubs: `skvideo.io.vread` returns the synthetic frames, the annotation pickles are not read (the object is
built without __init__).  The painting itself -- the draw of the annotation, the frame range, numpy's clipping of bbox[f, y:y+h, x:x+w] --
is the reference's code, executed as is.  No test needs this tool: tests/test_truth_boxes_cpu.py reads the recorded file."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402

H, W = 24, 32


def _still(n, box):
    return [list(box)] * n


def cases():
    """(F, [annotation (start, end, label, boxes (x, y, w, h) per frame from start, annotated frames)], seed)"""
    moving = [[2 + f, 1 + 2 * f, 9, 6] for f in range(12)]
    return [
        (8, [(0, 7, 3, _still(8, (5, 4, 10, 8)), [2, 5])], 11),                                   # a box inside the frame
        (8, [(0, 7, 1, _still(8, (25, 18, 12, 10)), [1])], 12),                                   # over the right and the bottom edge
        (8, [(0, 7, 2, _still(8, (-5, 3, 3, 7)), [0])], 13),                                      # negative x: the slice wraps to columns 27..29
        (8, [(0, 7, 2, [[-3, -4, 8, 3], [4, -3, 5, 6], [-40, 2, 45, 4], [-2, -2, 2, 2]] * 2, [3])], 14),   # wraps to empty, to a range, below -W
        (8, [(0, 7, 5, [[40, 2, 5, 5], [3, 30, 5, 5], [32, 24, 4, 4], [31, 23, 4, 4]] * 2, [])], 15),      # wholly outside; the last pixel
        (8, [(0, 7, 4, [[5, 5, 0, 6], [5, 5, 6, 0], [5, 5, 0, 0], [5, 5, 1, 1]] * 2, [4])], 16),  # zero w or h
        (12, [(3, 9, 7, moving[:7], [4, 6])], 17),                                                # start > 0
        (10, [(2, 20, 6, moving + moving[:7], [3])], 18),                                         # end beyond the video
        (9, [(0, 8, 8, _still(9, (1, 1, 6, 6)), [0]), (2, 6, 8, _still(5, (20, 10, 8, 9)), [3])], 19),          # two annotations: the draw matters
        (9, [(0, 8, 8, _still(9, (1, 1, 6, 6)), [0]), (2, 6, 8, _still(5, (20, 10, 8, 9)), [3])], 24),          # ... another seed, the other one
        (11, [(0, 4, 9, moving[:5], [1]), (1, 10, 9, _still(10, (-6, 20, 4, 9)), [5]), (5, 30, 9, moving[:6], [7])], 21),   # three
        (11, [(0, 4, 9, moving[:5], [1]), (1, 10, 9, _still(10, (-6, 20, 4, 9)), [5]), (5, 30, 9, moving[:6], [7])], 20),
        (11, [(0, 4, 9, moving[:5], [1]), (1, 10, 9, _still(10, (-6, 20, 4, 9)), [5]), (5, 30, 9, moving[:6], [7])], 25),
    ]


def main():
    ref_import.install_shims()
    store = {}
    sys.modules["skvideo.io"].vread = lambda path: store["frames"]
    mod = importlib.import_module("datasets.ucf_dataloader_eval")
    mod.vread = sys.modules["skvideo.io"].vread
    out = {"n": np.asarray(len(cases()))}
    for k, (F, anns, seed) in enumerate(cases()):
        store["frames"] = np.zeros((F, H, W, 3), np.uint8)
        ds = object.__new__(mod.UCF101DataLoader)
        ds._dataset_dir = "DATA_PATH"; ds.name = "test"
        np.random.seed(seed)
        video, bbox, label, _annot = ds.load_video("v%d" % k, anns)
        assert video.shape == (F, H, W, 3) and bbox.shape == (F, H, W, 1) and bbox.dtype == np.uint8
        out["shape_%d" % k] = np.asarray([F, H, W])
        out["seed_%d" % k] = np.asarray(seed)
        out["ann_%d" % k] = np.asarray([(a[0], a[1], a[2]) for a in anns], np.int64)
        for i, a in enumerate(anns):
            out["boxes_%d_%d" % (k, i)] = np.asarray(a[3], np.int64).reshape(-1, 4)
            out["annot_%d_%d" % (k, i)] = np.asarray(a[4], np.int64)
        out["bbox_%d" % k] = bbox[..., 0].copy()
        out["label_%d" % k] = np.asarray(label)
    path = os.path.join(ROOT, "tests", "golden", "eval_boxes.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), [int(out["bbox_%d" % k].sum()) for k in range(len(cases()))])


if __name__ == "__main__":
    main()
