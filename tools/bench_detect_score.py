#!/usr/bin/env python3
"""Scoring a finished detection pass against truth masks on one MI355X: detect.DetectEngine.score against the route a caller takes without it.

The synthetic uint8 videos, truth and labels of synthetic.make_eval_videos_u8 with frames of 240 x 320 and the synthetic weights, as the sibling
benches use them, on two engines: the centre crop (bs = 14) and tile + flip (8 views a clip, bs = 16).  After the pass every video's mask is
replaced by planted blob masks (three discs and twelve specks per frame, the masks of tools/bench_detect_instances.py): what a trained
model's output looks like.  Three ways to the evaluator's tables from the same finished pass:
  host          a synchronous .cpu() of every video's mask, intersection / union / truth counts per frame in numpy, detect.accumulate_video
  score         engine.score(truths, labels) with the truths on the host: each goes up through page-locked staging, one pc_map_crosstab
                launch per video, all tables down in one copy, one wait on the compute stream
  score_device  the same with the truths already on the device (a loader that keeps them there): nothing goes up
One warm-up, then `--passes` rounds that alternate the three; medians.  The tool asserts that the three give equal counts and equal tables.
bytes_to_host / bytes_to_device is what crosses PCIe; host_waits the synchronous waits of the host on the device.
Then pc_map_crosstab alone on F = 40 frames, 20 launches after 3 with device events around all 20, for P = 1 (blob masks against one
actor) and P = 8 (their map of ranks against three actors): microseconds, and GB/s of ALGORITHMIC bytes (both maps once, the tables) against
the 8 TB/s roof -- the maps are re-read launch after launch and are cache-resident: not an HBM rate.  Nothing is gated.

    python tools/bench_detect_score.py --out profiles/detect_score_bench.json [--videos 24] [--passes 5]
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
from picons_amd import detect, evalmetrics, ops, synthetic  # noqa: E402

ROOF_GBS = 8000.0


def blob_masks(F, H, W, seed):
    """Three discs and twelve specks per frame (tools/bench_detect_instances.py)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            m[f] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        m[f][rng.integers(0, H, 12), rng.integers(0, W, 12)] = 1
    return m


def engine_pass(de, videos):
    de.begin(True)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def host_route(de, truths, labels, dets):
    """What a caller does today: every mask to the host, the counts in numpy, the evaluator's accumulation restated."""
    acc = evalmetrics.MapAccumulator(de.C, device="cpu")
    counts = []
    for rec, t, lab, d in zip(de.videos, truths, labels, dets):
        m = rec.mask.cpu().numpy() != 0
        g = t.reshape(m.shape) != 0
        c = np.stack([(m & g).sum(axis=(1, 2)), (m | g).sum(axis=(1, 2)), g.sum(axis=(1, 2))], axis=1).astype(np.int64)
        counts.append(c)
        if c[:, 2].any():
            detect.accumulate_video(c, lab, acc)
            acc.n_correct += int(d.label == lab)
    return acc.result(), counts


def measure(de, truths, labels, dets, passes):
    dev_truths = [torch.from_numpy(t).to(de.dev) for t in truths]
    routes = (("host", lambda: host_route(de, truths, labels, dets)), ("score", lambda: de.score(truths, labels)),
              ("score_device", lambda: de.score(dev_truths, labels)))
    want, counts = routes[0][1]()                                    # warm-up, and what the others must equal
    equal = True
    for _name, fn in routes[1:]:
        ps = fn()
        equal = equal and all(np.array_equal(v.counts, c) for v, c in zip(ps.videos, counts))
        equal = equal and all(np.array_equal(np.asarray(ps.result[k]), np.asarray(want[k]), equal_nan=True) for k in want)
    times = {k: [] for k, _fn in routes}
    for _ in range(passes):
        for k, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    pixels = sum(t.size for t in truths)
    frames = sum(t.shape[0] for t in truths)
    n = len(truths)
    return dict(frames=frames, pixels=pixels, foreground_density=sum(int(c[:, 1].sum() - c[:, 2].sum() + c[:, 0].sum()) for c in counts) / pixels,
                seconds_median=med, seconds={k: sorted(v) for k, v in times.items()},
                score_over_host=med["host"] / med["score"], score_device_over_host=med["host"] / med["score_device"],
                bytes_to_host={"host": pixels, "score": 36 * frames, "score_device": 36 * frames},
                bytes_to_device={"host": 0, "score": pixels, "score_device": 0},
                host_waits={"host": n, "score": "1 on the compute stream, at most %d on the copy stream for its own uploads" % max(0, n - 2), "score_device": 1},
                fmAP_at_0_5=float(want["fmAP"][10]), vmAP_at_0_5=float(want["vmAP"][10]), equal=bool(equal))


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


def kernel_alone(pred, truth, P, A, what):
    F, H, W = (int(v) for v in pred.shape)
    out = torch.empty(F, P + 2, A + 2, dtype=torch.int32, device=pred.device)
    ws = torch.empty(ops.map_crosstab_ws_bytes(F, H, W, P, A), dtype=torch.uint8, device=pred.device)
    us = timed(lambda: ops.map_crosstab(pred, truth, P, A, out=out, ws=ws))
    got = out.cpu().numpy().astype(np.int64)
    p, t = pred.cpu().numpy().astype(np.int64), truth.cpu().numpy().astype(np.int64)
    pair = (np.minimum(p, P + 1) * (A + 2) + np.minimum(t, A + 1)).reshape(F, -1)
    want = np.stack([np.bincount(row, minlength=(P + 2) * (A + 2)) for row in pair]).reshape(F, P + 2, A + 2)
    b = 2 * F * H * W + 4 * F * (P + 2) * (A + 2)
    return dict(maps=what, frames=F, frame_hw=[H, W], P=P, A=A, blocks_per_frame=ws.numel() // (4 * F * (P + 2) * (A + 2)), launches=2,
                us_per_call=us, algorithmic_bytes=b, gb_per_s=b / us * 1e-3, fraction_of_8tbs_roof=b / us * 1e-3 / ROOF_GBS,
                equal_to_numpy=bool(np.array_equal(got, want)), bound="latency",
                note="two 240 x 320 x 40 maps are 6 MB and cache-resident, re-read by every launch: not an HBM rate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_score needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    made = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos, truths, labels = [v[0] for v in made], [np.ascontiguousarray(v[1][..., 0]) for v in made], [v[2] for v in made]
    state = synthetic.init_state(47, 24)
    report = {"metric": "seconds to score a finished detection pass against truth masks (blob masks, %d videos, frames %d x %d, centre crop)" % (a.videos, H, W),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W],
              "host": "a .cpu() of every mask, numpy counts, detect.accumulate_video", "score": "engine.score(truths, labels), truths on the host",
              "score_device": "engine.score(truths, labels), truths on the device", "gated": False}
    for name, kw in (("centre_crop", dict(bs=14)), ("tile_flip", dict(bs=16, tile=True, flip=True))):
        de = detect.DetectEngine(hw=hw, state=state, capacity=2048, **kw)
        dets = engine_pass(de, videos)
        for i, rec in enumerate(de.videos):                          # blob masks in place of what the synthetic weights give
            rec.mask.copy_(torch.from_numpy(blob_masks(rec.F, rec.H, rec.W, 7 + i)).to(rec.mask.device))
        torch.cuda.synchronize()
        report[name] = dict(measure(de, truths, labels, dets, a.passes), views=len(dets[0].views), clips=de.n_clips)
        del de
    report["value"] = report["centre_crop"]["seconds_median"]["score"]
    blob40 = torch.from_numpy(blob_masks(40, H, W, 7)).cuda()
    _inst, imap40 = ops.frame_instances(blob40, conn=8, min_area=1, K=8)
    one = torch.from_numpy(blob_masks(40, H, W, 11)).cuda()
    three = torch.from_numpy((blob_masks(40, H, W, 11) * np.random.default_rng(3).integers(1, 4, (40, 1, W))).astype(np.uint8)).cuda()
    report["kernel_alone_P1"] = kernel_alone(blob40, one, 1, 1, "blob masks against blob truth of one actor")
    report["kernel_alone_P8"] = kernel_alone(imap40, three, 8, 3, "their map of ranks against a truth of three actors")
    assert report["centre_crop"]["equal"] and report["tile_flip"]["equal"], "score() and the host route disagree"
    assert report["kernel_alone_P1"]["equal_to_numpy"] and report["kernel_alone_P8"]["equal_to_numpy"]
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
