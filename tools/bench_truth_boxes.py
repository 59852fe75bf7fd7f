#!/usr/bin/env python3
"""Truth given as boxes (evalstep.BoxTruth, pc_paint_boxes) against the dense truth routes on one MI355X.

The synthetic uint8 videos and labels of synthetic.make_eval_videos_boxes with frames of 240 x 320 and the synthetic weights, as
tools/bench_detect_score.py / bench_detect_sweep.py use them; the dense truths are the boxes' own dense().  Measured in THIS run, nothing taken
from an earlier file:
  score / sweep     DetectEngine.score and .sweep (19 thresholds) of one finished centre-crop pass (bs = 14, probabilities kept) three ways:
                    `boxes` (BoxTruth: the rect tables go up in one copy, each map is painted on the device), `dense_host` (uint8 maps on the host: each
                    goes up through page-locked staging) and `dense_device` (the maps already on the device: nothing goes up)
  eval              an EvalEngine pass (bs = 14, pack) over the same videos with box truths and with dense host truths: clips per second,
                    and the host's waits on a stream or an event per video, counted around add_video
  kernel_alone      pc_paint_boxes on 40 frames of 240 x 320 and on 2 frames of 1080 x 1920 (R = 2: a box and a pixel per frame; R = 32:
                    random rects) against torch.Tensor.zero_() of the same bytes, the write-bandwidth yardstick: 20 launches after 3 with
                    device events around all 20
One warm-up, then `--passes` rounds that alternate the routes; medians of host clocks around routes that end with the tables on the host.
The tool asserts that the routes give equal tables.  bytes_to_device is what crosses PCIe for the truths.  Nothing is gated.

    python tools/bench_truth_boxes.py --out profiles/truth_boxes_bench.json [--videos 24] [--passes 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import picons_amd  # noqa: F401,E402
from picons_amd import detect, evalstep, ops, synthetic  # noqa: E402

ROOF_GBS = 8000.0


def alternate(routes, passes):
    times = {k: [] for k, _fn in routes}
    for _ in range(passes):
        for k, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in times.items()}, {k: sorted(v) for k, v in times.items()}


def same_result(a, b):
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def measure_truth_calls(de, boxes, dense, labels, passes):
    dev = [torch.from_numpy(t).to(de.dev) for t in dense]
    out = {}
    for name, call, tables in (("score", lambda t: de.score(t, labels), lambda r: [v.table for v in r.videos]),
                               ("sweep", lambda t: de.sweep(t, labels), lambda r: r.videos)):
        routes = (("boxes", lambda: call(boxes)), ("dense_host", lambda: call(dense)), ("dense_device", lambda: call(dev)))
        got = [fn() for _k, fn in routes]                            # warm-up, and the tables that must agree
        equal = all(all(np.array_equal(x, y) for x, y in zip(tables(g), tables(got[1]))) for g in got)
        med, every = alternate(routes, passes)
        out[name] = dict(seconds_median=med, seconds=every, boxes_over_dense_host=med["dense_host"] / med["boxes"],
                         boxes_over_dense_device=med["dense_device"] / med["boxes"], equal=bool(equal))
    pixels, table = sum(t.size for t in dense), sum(b.nbytes for b in boxes)
    out["bytes_to_device"] = {"boxes": table, "dense_host": pixels, "dense_device": 0}
    out["frames"], out["rects_per_frame"] = sum(t.shape[0] for t in dense), int(boxes[0].rects.shape[1])
    return out


class WaitCounter:
    """Counts the host's waits on a stream or an event while it is on."""

    def __init__(self):
        self.n, self.on, self.real = 0, False, []
        for cls, name in ((torch.cuda.Event, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize")):
            real = getattr(cls, name)
            self.real.append((cls, name, real))
            setattr(cls, name, self._wrap(real))

    def _wrap(self, real):
        def f(*a, **k):
            self.n += int(self.on)
            return real(*a, **k)
        return f

    def restore(self):
        for cls, name, real in self.real:
            setattr(cls, name, real)


def measure_eval(state, hw, videos, boxes, dense, labels, passes):
    ee = evalstep.EvalEngine(bs=14, hw=hw, state=state, capacity=2048, pack=True)
    sets = {"boxes": list(zip(videos, boxes, labels)), "dense_host": list(zip(videos, dense, labels))}
    res = {k: ee.evaluate(v, pack=True) for k, v in sets.items()}     # warm-up
    clips = ee.n_clips
    med, every = alternate([(k, (lambda v: lambda: ee.evaluate(v, pack=True))(v)) for k, v in sets.items()], passes)
    wc = WaitCounter()
    waits = {}
    try:
        for k, v in sets.items():
            ee.begin(True)
            wc.n, wc.on = 0, True
            for f, t, lab in v:
                ee.add_video(f, t, lab)
            wc.on = False
            waits[k] = wc.n / len(v)
            ee.results()
    finally:
        wc.restore()
    frames_bytes = sum(v.nbytes for v in videos)
    return dict(clips=clips, videos=len(videos), skipped=ee.n_skipped, seconds_median=med, seconds=every,
                clips_per_s={k: clips / s for k, s in med.items()}, host_waits_per_video=waits,
                bytes_to_device={"boxes": frames_bytes + sum(b.nbytes for b in boxes), "dense_host": frames_bytes + sum(t.size for t in dense)},
                equal=bool(same_result(res["boxes"], res["dense_host"])))


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def kernel_alone(F, H, W, R, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros((F, R, 5), np.int64)
    if R == 2:                                                       # a box and a pixel per frame: what the annotations of a video look like
        for f in range(F):
            r[f, 0] = (W // 4 + f, W // 4 + f + W // 3, H // 4, H // 4 + H // 2, 1)
            r[f, 1] = (W // 2, W // 2 + 1, H // 2, H // 2 + 1, 1)
    else:
        r[..., 0:2] = np.sort(rng.integers(0, W + 1, (F, R, 2)), axis=2)
        r[..., 2:4] = np.sort(rng.integers(0, H + 1, (F, R, 2)), axis=2)
        r[..., 4] = rng.integers(1, 256, (F, R))
    bt = evalstep.BoxTruth((F, H, W), r)
    rects = torch.from_numpy(bt.rects).cuda()
    truth = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    us = timed(lambda: ops.paint_boxes(rects, F, H, W, truth=truth))
    equal = bool(np.array_equal(truth.cpu().numpy(), bt.dense()))
    fill = timed(lambda: truth.zero_())
    b = F * H * W
    return dict(frames=F, frame_hw=[H, W], R=R, bytes=b, paint_us=us, fill_us=fill, paint_over_fill=us / fill, paint_gb_per_s=b / us * 1e-3,
                fill_gb_per_s=b / fill * 1e-3, fraction_of_8tbs_roof=b / us * 1e-3 / ROOF_GBS, equal_to_numpy=equal,
                note="launch after launch over one buffer: a map of a few MB stays in the caches, so neither rate is an HBM rate; the fill is the yardstick")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_truth_boxes needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    made = synthetic.make_eval_videos_boxes(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos, boxes, labels = [v[0] for v in made], [v[1] for v in made], [v[2] for v in made]
    dense = [b.dense() for b in boxes]
    state = synthetic.init_state(47, 24)
    report = {"metric": "seconds to score a finished detection pass against truth given as boxes (%d videos, frames %d x %d, centre crop)" % (a.videos, H, W),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W], "gated": False}
    de = detect.DetectEngine(hw=hw, state=state, capacity=2048, bs=14)
    de.set_keep_probs(True)
    de.begin(True)
    for v in videos:
        de.add_video(v)
    de.results()
    report.update(measure_truth_calls(de, boxes, dense, labels, a.passes))
    del de
    report["eval"] = measure_eval(state, hw, videos, boxes, dense, labels, a.passes)
    report["kernel_alone"] = [kernel_alone(40, H, W, 2, 1), kernel_alone(40, H, W, 32, 2), kernel_alone(2, 1080, 1920, 2, 3), kernel_alone(2, 1080, 1920, 32, 4)]
    report["value"] = report["score"]["seconds_median"]["boxes"]
    assert report["score"]["equal"] and report["sweep"]["equal"] and report["eval"]["equal"], "the box routes and the dense routes disagree"
    assert all(k["equal_to_numpy"] for k in report["kernel_alone"])
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
