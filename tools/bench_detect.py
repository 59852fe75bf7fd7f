#!/usr/bin/env python3
"""Detection output on one MI355X: detect.DetectEngine against what a user had to do for detections before it existed.

Both paths get the same synthetic uint8 videos (synthetic.make_eval_videos_u8: frames of 240 x 256; the truth is not used) and the same weights:
  baseline   as of commit 4b9ddbe the only route to detections: an evalstep.EvalEngine pass with all-ones truth (so that every clip is kept)
             whose on_batch takes the logits of each batch -- sigmoid on the device, the copy of 1.6 MB per clip to the host, the threshold,
             the boxes and the undoing of the clip interleave in numpy
  engine     DetectEngine (pack off and on): pc_detect_frames behind each batch, the records read once per pass, the masks left on the device
One warm-up pass per path, then `--passes` rounds that alternate the paths; the median clips/s of each is reported, and the counts and boxes
of all paths must be equal.  Then pc_detect_frames alone (14 clips of 224 x 224 into frames of 240 x 256; device events, 20 launches after 3)
as GB/s of its algorithmic bytes -- 4 read per crop pixel, 1 written per frame pixel -- against the 8 TB/s roof.  The 22 MB of logits are
re-read every launch and fit the Infinity Cache, so the read side of that figure is not an HBM read.

    python tools/bench_detect.py --out profiles/detect_bench.json [--videos 24] [--passes 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import picons_amd  # noqa: F401,E402
from picons_amd import detect, evalstep, ops, synthetic  # noqa: E402

BASELINE_COMMIT = "4b9ddbe"
HBM_PEAK_GBS = 8000.0


def host_detections(engine, videos, hw):
    """The baseline: -> [(counts [F], boxes [F,4], masks [F,H,W] uint8 on the host)] per video."""
    out, todo = [], []

    def on_batch(m, logits, _scores):
        seg = torch.sigmoid(logits[:, 0]).cpu().numpy()                # (m, 8, hw, hw) float32: 1.6 MB per clip at 224
        pred = seg >= 0.5
        for j in range(m):
            vi, start = todo.pop(0)
            counts, boxes, masks = out[vi]
            F, H, W = masks.shape
            h0, w0 = evalstep.centre_crop(H, W, hw)
            for k in range(8):
                f = start + 2 * k
                if f >= F:
                    continue
                p = pred[j, k]
                masks[f, h0:h0 + hw, w0:w0 + hw] = p
                rows, cols = np.flatnonzero(p.any(1)), np.flatnonzero(p.any(0))
                counts[f] = int(p.sum())
                if rows.size:
                    boxes[f] = (w0 + cols[0], h0 + rows[0], w0 + cols[-1] + 1, h0 + rows[-1] + 1)

    engine.on_batch = on_batch
    engine.begin(pack=False)
    for vi, (frames, _truth, _label) in enumerate(videos):
        F, H, W = frames.shape[:3]
        out.append((np.zeros(F, np.int32), np.zeros((F, 4), np.int32), np.zeros((F, H, W), np.uint8)))
        todo += [(vi, s) for s in evalstep.clip_starts(F, np.ones(F))]
        engine.add_video(frames, np.ones((F, H, W), np.uint8), 0)
    engine.results()
    assert not todo
    return out


def kernel_rate(hw, n=14, device="cuda"):
    H, W = hw + 16, hw + 32
    F = 16 * (n // 2) + 16
    h0, w0 = evalstep.centre_crop(H, W, hw)
    starts = [(16 * (c // 2) + c % 2) for c in range(n)]
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(n, 8, hw, hw, generator=g) * 3).to(device)
    mask = torch.empty(F, H, W, dtype=torch.uint8, device=device)
    rec = torch.empty(F, 8, dtype=torch.int32, device=device)
    ws = torch.empty(ops.detect_frames_ws_bytes(n, hw), dtype=torch.uint8, device=device)
    fn = lambda: ops.detect_frames(logits, starts, F, H, W, h0, w0, mask=mask, rec=rec, ws=ws)
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 20
    nbytes = n * 8 * (4 * hw * hw + H * W)
    return dict(clips=n, frame_hw=[H, W], ms=ms, algorithmic_bytes=nbytes, bound="hbm", achieved=nbytes / 1e9 / (ms * 1e-3), peak=HBM_PEAK_GBS,
                unit="GB/s", frac=nbytes / 1e9 / (ms * 1e-3) / HBM_PEAK_GBS,
                note="two launches (frames, records); the %.1f MB of logits are re-read every launch and fit the Infinity Cache" % (n * 32 * hw * hw / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--bs", type=int, default=14)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect needs a GPU: nothing here is measured without one")
    hw = a.hw
    videos = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw)
    state = synthetic.init_state(47, 24)
    ee = evalstep.EvalEngine(bs=a.bs, hw=hw, state=state)
    de = detect.DetectEngine(bs=a.bs, hw=hw, state=state)

    def engine_pass(pack):
        de.begin(pack)
        for frames, _t, _l in videos:
            de.add_video(frames)
        return de.results()

    configs = {"baseline": lambda: host_detections(ee, videos, hw), "engine": lambda: engine_pass(False), "engine_packed": lambda: engine_pass(True)}
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = de.n_clips
    assert nclips == ee.n_clips
    base = results["baseline"]
    same = all(np.array_equal(d.counts, b[0]) and np.array_equal(d.boxes, b[1]) for k in ("engine", "engine_packed") for d, b in zip(results[k], base))
    same_masks = all(np.array_equal(d.masks.cpu().numpy(), b[2]) for d, b in zip(results["engine"], base))
    times = {k: [] for k in configs}
    for _ in range(a.passes):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                       # ends with the detections on the host (the engine's masks stay on the device)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    rate = {k: nclips / statistics.median(v) for k, v in times.items()}
    positive = sum(int(d.counts.sum()) for d in results["engine"])
    report = {
        "metric": "detection clips/sec from decoded uint8 video (bs=%d clips, 8x%dx%d, eval forward + masks, boxes, scores, class)" % (a.bs, hw, hw),
        "value": rate["engine"], "unit": "clips/s", "videos": a.videos, "clips": nclips, "passes": a.passes,
        "baseline": "EvalEngine pass as of commit %s with all-ones truth; on_batch: sigmoid, copy to the host, threshold, numpy boxes and "
                    "de-interleaving" % BASELINE_COMMIT,
        "clips_per_s": rate, "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "engine_over_baseline": rate["engine"] / rate["baseline"], "engine_packed_over_baseline": rate["engine_packed"] / rate["baseline"],
        "same_counts_and_boxes": bool(same), "same_masks": bool(same_masks), "positive_pixels": positive,
        "tubes": sum(len(d.tubes()) for d in results["engine"]),
        "kernels": {"detect_frames": kernel_rate(hw, a.bs if a.bs <= 32 else 14)},
    }
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_detect: the engine's counts and boxes differ from the host path's")


if __name__ == "__main__":
    main()
