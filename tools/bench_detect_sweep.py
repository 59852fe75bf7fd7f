#!/usr/bin/env python3
"""Scoring a finished detection pass at every mask threshold on one MI355X: detect.DetectEngine.sweep against the routes a caller takes
without it, and what keeping the probability map costs a pass.

The synthetic uint8 videos, truth and labels of synthetic.make_eval_videos_u8 with frames of 240 x 256 and the synthetic weights on the
centre-crop engine (bs = 14).  After a pass with set_keep_probs(True) every video's probability map is replaced by a planted one -- three
discs a frame whose probability falls off towards the rim over a background below 0.05, and its mask by that map cut at word 32768: what a
trained model's output looks like (the synthetic weights give a map that hovers around one value).  From the same finished pass:
  host          what a caller does today for N thresholds: a synchronous .cpu() of every video's probability map (2 bytes a pixel), per
                threshold `>=` and the intersection / union / truth counts in numpy, detect.accumulate_video
  sweep         engine.sweep(truths, labels) at the default N = 19 with the truths on the host: each goes up through page-locked staging,
                one pc_prob_truth_hist launch per video, all histograms down in one copy, one wait on the compute stream
  sweep_device  the same with the truths already on the device
  score         engine.score(truths, labels): the cost of ONE threshold today
One warm-up, then `--passes` rounds that alternate the four; medians and ranges.  The tool asserts that host and sweep give equal counts at
every threshold and that threshold 0.5 of the sweep is score()'s result.
Then the pass itself, `--passes` rounds alternating set_keep_probs(False) and (True): begin .. results() around a device synchronise.
Then pc_prob_truth_hist alone at N = 19 on one 40-frame video next to pc_map_crosstab at P = A = 1 on the same frames (the mask of the map),
20 launches after 3 with device events around all 20, for the planted map and for a map of noise: microseconds, and GB/s of ALGORITHMIC
bytes (3 a pixel against 2) against the 8 TB/s roof -- the maps are re-read launch after launch and are cache-resident: not an HBM rate.
Nothing is gated.

    python tools/bench_detect_sweep.py --out profiles/detect_sweep_bench.json [--videos 24] [--passes 5]
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


def blob_probs(F, H, W, seed):
    """uint16 [F, H, W]: three discs per frame, 0.98 at the centre falling linearly to 0.3 at the rim, over a background of 0 .. 0.04."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    p = rng.random((F, H, W)) * 0.04
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            d = np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) / r
            p[f] = np.where(d <= 1.0, np.maximum(p[f], 0.98 - 0.68 * d), p[f])
    return np.rint(p * 65535.0).astype(np.uint16)


def to_prob_tensor(q, dev):
    return torch.from_numpy(q.view(np.int16)).to(dev)


def engine_pass(de, videos):
    de.begin(True)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def host_route(de, truths, labels, dets, words):
    """What a caller does today: every probability map to the host, per threshold the counts in numpy, the evaluator's accumulation restated."""
    accs = [evalmetrics.MapAccumulator(de.C, device="cpu") for _ in words]
    counts = []
    for rec, t, lab, d in zip(de.videos, truths, labels, dets):
        q = rec.prob.cpu().numpy().view(np.uint16)
        g = t.reshape(q.shape) != 0
        gt = g.sum(axis=(1, 2))
        per = []
        for k, w in enumerate(words):
            m = q >= w
            c = np.stack([(m & g).sum(axis=(1, 2)), (m | g).sum(axis=(1, 2)), gt], axis=1).astype(np.int64)
            per.append(c)
            if gt.any():
                detect.accumulate_video(c, lab, accs[k])
                accs[k].n_correct += int(d.label == lab)
        counts.append(np.stack(per))
    return [a.result() for a in accs], counts


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def measure(de, truths, labels, dets, passes):
    words = detect.threshold_words()
    N = int(words.size)
    dev_truths = [torch.from_numpy(t).to(de.dev) for t in truths]
    routes = (("host", lambda: host_route(de, truths, labels, dets, words.tolist())), ("sweep", lambda: de.sweep(truths, labels)),
              ("sweep_device", lambda: de.sweep(dev_truths, labels)), ("score", lambda: de.score(truths, labels)))
    want, counts = routes[0][1]()                                    # warm-up, and what the sweeps must equal
    equal = True
    for _name, fn in routes[1:3]:
        sw = fn()
        equal = equal and all(np.array_equal(detect.sweep_counts(h), c) for h, c in zip(sw.videos, counts))
        equal = equal and all(np.array_equal(np.asarray(sw.results[k][key]), np.asarray(want[k][key]), equal_nan=True) for k in range(N) for key in want[k])
    ps = routes[3][1]()
    half = int(np.flatnonzero(words == 32768)[0])
    equal = equal and all(np.array_equal(np.asarray(ps.result[key]), np.asarray(sw.results[half][key]), equal_nan=True) for key in ps.result)
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
    with np.errstate(invalid="ignore", divide="ignore"):
        fm = [float(np.nanmean(r["frame_ious"] / r["n_tot_frames"], axis=0)[10]) for r in sw.results]
    return dict(frames=frames, pixels=pixels, thresholds=N, seconds=dict((k, spread(v)) for k, v in times.items()), seconds_all={k: sorted(v) for k, v in times.items()},
                sweep_over_host=med["host"] / med["sweep"], sweep_device_over_host=med["host"] / med["sweep_device"],
                sweep_over_one_score=med["sweep"] / med["score"], sweep_over_n_scores=med["sweep"] / (N * med["score"]),
                bytes_to_host={"host": 2 * pixels, "sweep": 8 * (N + 1) * frames, "sweep_device": 8 * (N + 1) * frames, "score": 36 * frames},
                bytes_to_device={"host": 0, "sweep": pixels, "sweep_device": 0, "score": pixels},
                host_waits={"host": n, "sweep": "1 on the compute stream, at most %d on the copy stream for its own uploads" % max(0, n - 2), "sweep_device": 1,
                            "score": "as sweep"},
                fmAP_at_0_5_over_classes_with_a_video=fm, pixel_tp_fp_fn=sw.pixel.tolist(), equal=bool(equal))


def keep_cost(de, videos, passes):
    """A whole pass, begin .. results() and a device synchronise, with and without the probability map kept; alternating."""
    times = {False: [], True: []}
    for keep in (False, True):                                       # warm-up of both
        de.set_keep_probs(keep)
        engine_pass(de, videos)
    for _ in range(passes):
        for keep in (False, True):
            de.set_keep_probs(keep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            engine_pass(de, videos)
            torch.cuda.synchronize()
            times[keep].append(time.perf_counter() - t0)
    off, on = statistics.median(times[False]), statistics.median(times[True])
    return dict(seconds_without=spread(times[False]), seconds_with=spread(times[True]), seconds_all={"without": sorted(times[False]), "with": sorted(times[True])},
                with_over_without=on / off, clips=de.n_clips,
                note="with: one pc_frame_probs launch behind each pc_detect_frames and 2 bytes a pixel of device memory per video until the next begin()")


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


def kernels_alone(q, truth, words, what):
    """pc_prob_truth_hist at the words and pc_map_crosstab at P = A = 1 on the mask of the same map, the same frames and truth."""
    F, H, W = q.shape
    N = len(words)
    dev = "cuda"
    prob, tr = to_prob_tensor(q, dev), torch.from_numpy(truth).to(dev)
    mask = torch.from_numpy((q >= 32768).astype(np.uint8)).to(dev)
    out_h = torch.empty(F, 2, N + 1, dtype=torch.int32, device=dev)
    ws_h = torch.empty(ops.prob_truth_hist_ws_bytes(F, H, W, N), dtype=torch.uint8, device=dev)
    out_c = torch.empty(F, 3, 3, dtype=torch.int32, device=dev)
    ws_c = torch.empty(ops.map_crosstab_ws_bytes(F, H, W, 1, 1), dtype=torch.uint8, device=dev)
    us = {"hist": [], "crosstab": []}
    for _ in range(3):                                               # alternating, three windows of 20 launches each
        us["hist"].append(timed(lambda: ops.prob_truth_hist(prob, tr, words, out=out_h, ws=ws_h)))
        us["crosstab"].append(timed(lambda: ops.map_crosstab(mask, tr, 1, 1, out=out_c, ws=ws_c)))
    got = out_h.cpu().numpy()
    b = np.searchsorted(np.asarray(words, np.int64), q.astype(np.int64), side="right")
    cell = ((truth != 0).astype(np.int64) * (N + 1) + b).reshape(F, -1)
    want = np.stack([np.bincount(row, minlength=2 * (N + 1)) for row in cell]).reshape(F, 2, N + 1)
    hb, cb = 3 * F * H * W + 8 * F * (N + 1), 2 * F * H * W + 36 * F
    h, c = statistics.median(us["hist"]), statistics.median(us["crosstab"])
    return dict(maps=what, frames=F, frame_hw=[H, W], thresholds=N, blocks_per_frame=ws_h.numel() // (8 * F * (N + 1)), launches=2,
                pixels_at_or_above_the_first_word=float((q >= words[0]).mean()), truth_density=float((truth != 0).mean()),
                hist_us=spread(us["hist"]), crosstab_us=spread(us["crosstab"]), hist_over_crosstab=h / c, byte_ratio=hb / cb,
                hist_algorithmic_bytes=hb, hist_gb_per_s=hb / h * 1e-3, hist_fraction_of_8tbs_roof=hb / h * 1e-3 / ROOF_GBS,
                crosstab_algorithmic_bytes=cb, crosstab_gb_per_s=cb / c * 1e-3,
                equal_to_numpy=bool(np.array_equal(got, want)),
                note="a 240 x 256 x 40 map and its truth are 7 MB and cache-resident, re-read by every launch: not an HBM rate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_sweep needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 32
    made = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos, truths, labels = [v[0] for v in made], [np.ascontiguousarray(v[1][..., 0]) for v in made], [v[2] for v in made]
    state = synthetic.init_state(47, 24)
    report = {"metric": "seconds to score a finished detection pass at 19 mask thresholds (planted probability maps, %d videos, frames %d x %d, centre crop)" % (a.videos, H, W),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W],
              "host": "a .cpu() of every probability map, numpy >= and counts per threshold, detect.accumulate_video",
              "sweep": "engine.sweep(truths, labels), truths on the host", "sweep_device": "engine.sweep(truths, labels), truths on the device",
              "score": "engine.score(truths, labels): one threshold", "gated": False}
    de = detect.DetectEngine(hw=hw, state=state, capacity=2048, bs=14)
    report["keep_probs"] = keep_cost(de, videos, a.passes)
    de.set_keep_probs(True)
    dets = engine_pass(de, videos)
    for i, rec in enumerate(de.videos):                              # planted maps in place of what the synthetic weights give, and their masks
        q = blob_probs(rec.F, rec.H, rec.W, 7 + i)
        rec.prob.copy_(to_prob_tensor(q, rec.prob.device))
        rec.mask.copy_(torch.from_numpy((q >= 32768).astype(np.uint8)).to(rec.mask.device))
    torch.cuda.synchronize()
    report["centre_crop"] = dict(measure(de, truths, labels, dets, a.passes), views=len(dets[0].views), clips=de.n_clips)
    report["value"] = report["centre_crop"]["seconds"]["sweep"]["median"]
    words = detect.threshold_words().tolist()
    truth40 = (blob_probs(40, H, W, 11) >= 32768).astype(np.uint8)
    report["kernel_alone_blobs"] = kernels_alone(blob_probs(40, H, W, 7), truth40, words, "planted discs over a background below the first word")
    rng = np.random.default_rng(3)
    report["kernel_alone_noise"] = kernels_alone(rng.integers(0, 65536, (40, H, W)).astype(np.uint16), (rng.random((40, H, W)) < 0.5).astype(np.uint8), words,
                                                 "uniform noise, truth of density 0.5: the cell changes at nearly every pixel")
    assert report["centre_crop"]["equal"], "sweep() and the host route disagree"
    assert report["kernel_alone_blobs"]["equal_to_numpy"] and report["kernel_alone_noise"]["equal_to_numpy"]
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
