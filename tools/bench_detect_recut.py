#!/usr/bin/env python3
"""Cutting a finished detection pass again at another mask threshold on one MI355X: detect.DetectEngine.recut against the routes a caller
takes without it, and what detecting at a threshold costs a pass.

The 24 synthetic uint8 videos of tools/bench_detect_sweep.py (frames of 240 x 256, the synthetic weights, the centre-crop engine at bs = 14)
with its planted probability maps: after a pass with set_keep_probs(True) every video's map is replaced by three discs a frame whose
probability falls off towards the rim, and its mask by that map cut at word 32768.  At the threshold --threshold (0.35):
  (a) host        what a caller does today: a synchronous .cpu() of every video's probability map (2 bytes a pixel), `>=` in numpy, counts and
                  boxes in numpy
      recut       engine.recut(t): one pc_prob_cut launch per video, the records down in one copy each, one wait on the compute stream
  (b) second_pass a second full pass under set_mask_threshold(t), begin .. results(), on a second engine (its maps are the synthetic weights')
  (c) keep_pass   the same packed pass with set_keep_probs(True) only: second_pass over keep_pass is the price of the extra launch
One warm-up, then `--passes` rounds that alternate the four -- the two passes swap places every round, so that neither always runs behind the
host route --; medians and ranges.  The tool asserts that host and recut give equal counts and
boxes.
  (d) pc_prob_cut alone on one 40-frame video next to pc_prob_truth_hist at N = 1 on the same frames, 20 launches after 3 with device events
      around all 20, three windows each, alternating, for the planted map and for a map of noise.  Both move 3 ALGORITHMIC bytes a pixel (2 read
      + 1 written, against 3 read): microseconds and their ratio.  The maps are re-read launch after launch and are cache-resident: not an
      HBM rate.
Nothing is gated.

    python tools/bench_detect_recut.py --out profiles/detect_recut_bench.json [--videos 24] [--passes 6] [--threshold 0.35]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import picons_amd  # noqa: F401,E402
from picons_amd import detect, ops, synthetic  # noqa: E402
from bench_detect_sweep import blob_probs, engine_pass, spread, timed, to_prob_tensor  # noqa: E402


def host_route(de, word):
    """What a caller does today: every probability map to the host, the mask, the counts and the boxes in numpy."""
    out = []
    for rec in de.videos:
        q = rec.prob.cpu().numpy().view(np.uint16)
        m = q >= word
        counts = m.sum(axis=(1, 2))
        rows, cols = m.any(axis=2), m.any(axis=1)
        boxes = np.zeros((rec.F, 4), np.int64)
        for f in np.flatnonzero(counts):
            ys, xs = np.flatnonzero(rows[f]), np.flatnonzero(cols[f])
            boxes[f] = [xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]
        out.append((m.astype(np.uint8), counts, boxes))
    return out


def timed_pass(de, videos):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    engine_pass(de, videos)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(de, de2, videos, t, passes):
    word = detect.cut_word(t)

    def keep_pass():
        de2.set_mask_threshold(None)
        de2.set_keep_probs(True)
        return timed_pass(de2, videos)

    def threshold_pass():
        de2.set_keep_probs(False)
        de2.set_mask_threshold(t)
        return timed_pass(de2, videos)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    want = host_route(de, word)                                       # warm-up, and what the recut must equal
    dets = de.recut(t)
    equal = all(np.array_equal(d.counts, c) and np.array_equal(d.boxes, b) and np.array_equal(d.masks.cpu().numpy(), m) for d, (m, c, b) in zip(dets, want))
    keep_pass(), threshold_pass()
    times = dict(host=[], recut=[], second_pass=[], keep_pass=[])
    for i in range(passes):
        times["host"].append(wall(lambda: host_route(de, word)))
        times["recut"].append(wall(lambda: de.recut(t)))
        for name, fn in (("keep_pass", keep_pass), ("second_pass", threshold_pass))[::1 if i % 2 == 0 else -1]:      # the two passes swap places every round
            times[name].append(fn())
    med = {k: statistics.median(v) for k, v in times.items()}
    pixels = sum(r.F * r.H * r.W for r in de.videos)
    frames = sum(r.F for r in de.videos)
    return dict(threshold=t, word=word, frames=frames, pixels=pixels, positive_fraction=float(sum(int(c.sum()) for _m, c, _b in want)) / pixels,
                seconds=dict((k, spread(v)) for k, v in times.items()), seconds_all={k: sorted(v) for k, v in times.items()},
                host_over_recut=med["host"] / med["recut"], second_pass_over_recut=med["second_pass"] / med["recut"],
                second_pass_over_keep_pass=med["second_pass"] / med["keep_pass"], clips=de2.n_clips,
                bytes_to_host={"host": 2 * pixels, "recut": 4 * sum(r.dev.numel() for r in de.videos)},
                host_waits={"host": len(de.videos), "recut": 1}, equal=bool(equal),
                note="second_pass and keep_pass run on a second engine whose maps are the synthetic weights' (they hover around one value); "
                     "recut and host run on the planted maps")


def kernels_alone(q, word, what):
    """pc_prob_cut at the word and pc_prob_truth_hist at the one word on the same map, with the map's own mask as the truth."""
    F, H, W = q.shape
    dev = "cuda"
    prob = to_prob_tensor(q, dev)
    tr = torch.from_numpy((q >= word).astype(np.uint8)).to(dev)
    mask = torch.empty(F, H, W, dtype=torch.uint8, device=dev)
    rec = torch.zeros(F, 8, dtype=torch.int32, device=dev)
    ws_c = torch.empty(ops.prob_cut_ws_bytes(F, H, W), dtype=torch.uint8, device=dev)
    out_h = torch.empty(F, 2, 2, dtype=torch.int32, device=dev)
    ws_h = torch.empty(ops.prob_truth_hist_ws_bytes(F, H, W, 1), dtype=torch.uint8, device=dev)
    us = {"cut": [], "cut_records_only": [], "hist": []}
    for _ in range(3):                                               # alternating, three windows of 20 launches each
        us["cut"].append(timed(lambda: ops.prob_cut(prob, word, mask=mask, rec=rec, ws=ws_c)))
        us["hist"].append(timed(lambda: ops.prob_truth_hist(prob, tr, [word], out=out_h, ws=ws_h)))
        us["cut_records_only"].append(timed(lambda: ops.prob_cut(prob, word, rec=rec, ws=ws_c, want_mask=False)))
    equal = bool(np.array_equal(mask.cpu().numpy(), (q >= word).astype(np.uint8)) and np.array_equal(rec[:, 0].cpu().numpy(), (q >= word).sum(axis=(1, 2))))
    c, h = statistics.median(us["cut"]), statistics.median(us["hist"])
    nbytes = 3 * F * H * W
    return dict(maps=what, frames=F, frame_hw=[H, W], word=word, blocks_per_frame=ws_c.numel() // (32 * F), launches=2,
                positive_fraction=float((q >= word).mean()), cut_us=spread(us["cut"]), cut_records_only_us=spread(us["cut_records_only"]),
                hist_us=spread(us["hist"]), cut_over_hist=c / h, algorithmic_bytes=nbytes, cut_gb_per_s=nbytes / c * 1e-3, hist_gb_per_s=nbytes / h * 1e-3,
                equal_to_numpy=equal,
                note="a 240 x 256 x 40 map and its mask are 7 MB and cache-resident, re-read by every launch: not an HBM rate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=6)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--threshold", type=float, default=0.35)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_recut needs a GPU: nothing here is measured without one")
    hw, t = a.hw, a.threshold
    H, W = hw + 16, hw + 32
    made = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos = [v[0] for v in made]
    state = synthetic.init_state(47, 24)
    report = {"metric": "seconds to cut a finished detection pass again at a mask threshold (planted probability maps, %d videos, frames %d x %d, centre crop)" % (a.videos, H, W),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W],
              "host": "a .cpu() of every probability map, numpy >=, counts and boxes in numpy", "recut": "engine.recut(t)",
              "second_pass": "a second full packed pass under set_mask_threshold(t)", "keep_pass": "the same pass with set_keep_probs(True) only",
              "gated": False}
    de = detect.DetectEngine(hw=hw, state=state, capacity=2048, bs=14)
    de.set_keep_probs(True)
    engine_pass(de, videos)
    for i, rec in enumerate(de.videos):                              # planted maps in place of what the synthetic weights give, and their masks
        q = blob_probs(rec.F, rec.H, rec.W, 7 + i)
        rec.prob.copy_(to_prob_tensor(q, rec.prob.device))
        rec.mask.copy_(torch.from_numpy((q >= 32768).astype(np.uint8)).to(rec.mask.device))
    torch.cuda.synchronize()
    de2 = detect.DetectEngine(hw=hw, state=state, capacity=2048, bs=14)
    report["centre_crop"] = measure(de, de2, videos, t, a.passes)
    report["value"] = report["centre_crop"]["seconds"]["recut"]["median"]
    word = detect.cut_word(t)
    report["kernel_alone_blobs"] = kernels_alone(blob_probs(40, H, W, 7), word, "planted discs over a background below the word")
    rng = np.random.default_rng(3)
    report["kernel_alone_noise"] = kernels_alone(rng.integers(0, 65536, (40, H, W)).astype(np.uint16), word, "uniform noise: about two pixels in three positive")
    assert report["centre_crop"]["equal"], "recut() and the host route disagree"
    assert report["kernel_alone_blobs"]["equal_to_numpy"] and report["kernel_alone_noise"]["equal_to_numpy"]
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
