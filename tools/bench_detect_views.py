#!/usr/bin/env python3
"""Multi-view detection on one MI355X: detect.DetectEngine with tile / flip views against the centre-crop path and against what a user had to
write for the same merge without the two view kernels.

Every configuration gets the same synthetic uint8 videos (synthetic.make_eval_videos_u8 with frames of 240 x 320, or 240 x 256 with --narrow;
the truth is not used) and the same weights, each at a bs that is a multiple of its views per clip:
  centre       the path of the parent commit 96984af: the centre crop alone, pc_clips_from_u8 + pc_detect_frames
  tile         make_views(tile=True): the whole frame as overlapping tiles
  flip         the centre crop and its mirror image
  tile_flip    both
  torch_merge  the baseline for tile_flip: the same engine, cut and forward, its merge launch taken out; on_batch adds the views' logits into
               full-frame float32 buffers with torch ops on the device (slices, .flip), divides by the cover count, thresholds the sigmoid,
               copies the masks to the host and takes counts and boxes in numpy
One warm-up pass per configuration, then `--passes` rounds that alternate them; medians.  clips/s counts the video's clips (a clip of V views
is V forwards).  Nothing is gated.  Then each new kernel alone (device events, 20 launches after 3) as GB/s of its algorithmic bytes against
the 8 TB/s roof: the cut reads 3 B and writes 16 B per view pixel, the merge reads 4 B per view pixel and writes 1 B per frame pixel.  The
sources of both (a video of a few MB, the logits of one batch) are re-read every launch and fit the Infinity Cache: those reads are not HBM
reads.

    python tools/bench_detect_views.py --out profiles/detect_views_bench.json [--videos 24] [--passes 5] [--narrow]
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

PARENT_COMMIT = "96984af"
HBM_PEAK_GBS = 8000.0


def engine_pass(de, videos):
    de.begin(False)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def torch_merge_pass(de, videos, hw):
    """The baseline -> [(counts [F], boxes [F,4])] per video.  `de` is a views engine whose _collect does nothing."""
    out, todo, bufs = [], [], {}

    def finish(vi):
        acc, num = bufs.pop(vi)
        merged = acc / num.clamp(min=1).float()
        masks = ((torch.sigmoid(merged) >= 0.5) & (num > 0)).to(torch.uint8).cpu().numpy()
        counts, boxes = out[vi]
        for f in range(masks.shape[0]):
            p = masks[f] != 0
            rows, cols = np.flatnonzero(p.any(1)), np.flatnonzero(p.any(0))
            counts[f] = int(p.sum())
            if rows.size:
                boxes[f] = (cols[0], rows[0], cols[-1] + 1, rows[-1] + 1)

    def on_batch(m, logits, _scores):
        vi, st, views, last = todo.pop(0)
        n, V = len(st), len(views)
        lg = logits[:, 0].view(V, n, 8, hw, hw)
        acc, num = bufs[vi]
        F = acc.shape[0]
        for c, s in enumerate(st):
            K = len(range(s, min(F, s + 16), 2))
            for v, (h0, w0, fl) in enumerate(views):
                t = lg[v, c, :K]
                acc[s:s + 2 * K:2, h0:h0 + hw, w0:w0 + hw] += t.flip(-1) if fl else t
                num[s:s + 2 * K:2, h0:h0 + hw, w0:w0 + hw] += 1
        if last:
            finish(vi)

    de.on_batch = on_batch
    de.begin(False)
    for vi, frames in enumerate(videos):
        F, H, W = frames.shape[:3]
        views = de.video_views(H, W)
        per = de.bs // len(views)
        starts = evalstep.clip_starts(F, np.ones(F))
        out.append((np.zeros(F, np.int32), np.zeros((F, 4), np.int32)))
        bufs[vi] = (torch.zeros(F, H, W, device=de.dev), torch.zeros(F, H, W, dtype=torch.int32, device=de.dev))
        todo += [(vi, starts[i:i + per], views, i + per >= len(starts)) for i in range(0, len(starts), per)]
        de.add_video(frames)
    de.results()
    assert not todo and not bufs
    return out


def _time(fn):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 20


def kernel_rates(hw, H, W, views, n, device="cuda"):
    V = len(views)
    F = 16 * ((n + 1) // 2)
    starts = [(16 * (c // 2) + c % 2) for c in range(n)]
    g = torch.Generator().manual_seed(1)
    video = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).to(device)
    data = torch.empty(V, n, 8, hw, hw, 4, device=device)
    ms_cut = _time(lambda: ops.clips_from_u8_views(video, views, hw, starts, out=data))
    logits = (torch.randn(V, n, 8, hw, hw, generator=g) * 3).to(device)
    mask = torch.empty(F, H, W, dtype=torch.uint8, device=device)
    rec = torch.empty(F, 8, dtype=torch.int32, device=device)
    ws = torch.empty(ops.detect_frames_views_ws_bytes(n, H, W), dtype=torch.uint8, device=device)
    ms_merge = _time(lambda: ops.detect_frames_views(logits, views, starts, F, H, W, mask=mask, rec=rec, ws=ws))
    out = {}
    for name, ms, nbytes, note in (
            ("clips_from_u8_views", ms_cut, V * n * 8 * hw * hw * 19,
             "the %.1f MB video is re-read every launch and fits the Infinity Cache: its reads are not HBM reads" % (video.numel() / 1e6)),
            ("detect_frames_views", ms_merge, n * 8 * (V * 4 * hw * hw + H * W),
             "two launches (frames, records); the %.1f MB of logits are re-read every launch and fit the Infinity Cache: not HBM reads" % (logits.numel() * 4 / 1e6))):
        out[name] = dict(views=V, clips=n, frame_hw=[H, W], ms=ms, algorithmic_bytes=nbytes, bound="hbm", achieved=nbytes / 1e9 / (ms * 1e-3),
                         peak=HBM_PEAK_GBS, unit="GB/s", frac=nbytes / 1e9 / (ms * 1e-3) / HBM_PEAK_GBS, note=note)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--narrow", action="store_true", help="frames of hw + 16 by hw + 32 (240 x 256) instead of 240 x 320")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_views needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = (hw + 16, hw + 32) if a.narrow else (hw + 16, hw + 96)
    videos = [v[0] for v in synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))]
    state = synthetic.init_state(47, 24)
    kinds = {"centre": dict(), "tile": dict(tile=True), "flip": dict(flip=True), "tile_flip": dict(tile=True, flip=True)}
    nviews = {k: len(detect.make_views(H, W, hw, **kw)) for k, kw in kinds.items()}
    bs = {k: (14 if v <= 2 else -(-12 // v) * v) for k, v in nviews.items()}      # 14 as tools/bench_detect.py; else the multiple of V from 12 up
    engines = {k: detect.DetectEngine(bs=bs[k], hw=hw, state=state, capacity=1024, **kw) for k, kw in kinds.items()}
    base = detect.DetectEngine(bs=bs["tile_flip"], hw=hw, state=state, capacity=1024, masks=False, **kinds["tile_flip"])
    base._collect = lambda *args: None                                 # the merge launch taken out: the baseline's on_batch does its work
    configs = {k: (lambda de=de: engine_pass(de, videos)) for k, de in engines.items()}
    configs["torch_merge"] = lambda: torch_merge_pass(base, videos, hw)
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = engines["centre"].n_clips
    assert all(de.n_clips == nclips for de in engines.values()) and base.n_clips == nclips
    same = all(np.array_equal(d.counts, b[0]) and np.array_equal(d.boxes, b[1]) for d, b in zip(results["tile_flip"], results["torch_merge"]))
    times = {k: [] for k in configs}
    for _ in range(a.passes):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                       # ends with the detections on the host (the engines' masks stay on the device)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    report = {
        "metric": "multi-view detection clips/sec from decoded uint8 video (frames %d x %d, 8x%dx%d views, eval forward + merged masks, boxes, scores, "
                  "class)" % (H, W, hw, hw),
        "value": nclips / med["tile_flip"], "unit": "clips/s", "videos": a.videos, "clips": nclips, "passes": a.passes, "frame_hw": [H, W],
        "centre": "the parent commit's (%s) path: pc_clips_from_u8 + pc_detect_frames on the centre crop" % PARENT_COMMIT,
        "baseline": "torch_merge: the tile_flip engine without its merge launch; on_batch merges with torch ops on the device, boxes on the host",
        "views_per_clip": nviews, "bs": dict(bs, torch_merge=bs["tile_flip"]),
        "clips_per_s": {k: nclips / v for k, v in med.items()},
        "views_per_s": {k: nclips * nviews.get(k, nviews["tile_flip"]) / v for k, v in med.items()},
        "pass_seconds_median": med, "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "tile_flip_over_torch_merge": med["torch_merge"] / med["tile_flip"],
        "same_counts_and_boxes_as_torch_merge": bool(same),
        "positive_pixels": {k: sum(int(d.counts.sum()) for d in results[k]) for k in kinds},
        "kernels": kernel_rates(hw, H, W, detect.make_views(H, W, hw, tile=True, flip=True), bs["tile_flip"] // nviews["tile_flip"]),
        "gated": False,
    }
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
