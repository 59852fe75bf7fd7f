#!/usr/bin/env python3
"""A confidence per instance on one MI355X: detect.DetectEngine(instance_scores=True) against the engine without it.

Both configurations get the same synthetic uint8 videos (synthetic.make_eval_videos_u8 with frames of 240 x 320; the truth is not used) and
the same weights, at pack=True and pack=False:
  parent   the path of the parent commit 8846cf3: DetectEngine(instances=8, instance_maps=True)
  scores   the same engine with instance_scores=True: one pc_frame_probs launch behind every pc_detect_frames, one pc_instance_scores launch
           per video behind pc_frame_instances, the records in the same copy
One warm-up pass per configuration, then `--passes` rounds that alternate them; medians.  The tool checks that every existing field is equal.
Then the two kernels alone, 20 launches after 3 with device events around all 20: pc_frame_probs at the tile + flip shape (V = 8 views of
n = 2 clips, S = 224, frames of 240 x 320) and pc_instance_scores on planted blob masks (F = 40, K = 8, the masks of
tools/bench_detect_instances.py).  Each is given in microseconds and as GB/s of ALGORITHMIC bytes (the logits a merged pixel needs and the 2
bytes it writes; the map byte, the 2 probability bytes of a foreground pixel and the record) against the 8 TB/s roof -- but the inputs are
re-read launch after launch and are cache-resident, as they are in the engine, where the detect launch in front has just read the same
logits: the figure is not an HBM rate.  Nothing is gated.

    python tools/bench_instance_scores.py --out profiles/instance_scores_bench.json [--videos 24] [--passes 5]
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
from picons_amd import detect, ops, synthetic  # noqa: E402

PARENT_COMMIT = "8846cf3"
K, CONN, MIN_AREA = 8, 8, 1
ROOF_GBS = 8000.0


def engine_pass(de, videos, pack):
    de.begin(pack)
    for frames in videos:
        de.add_video(frames)
    return de.results()


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


def probs_alone(H=240, W=320, S=224, n=2, device="cuda"):
    views = detect.make_views(H, W, S, tile=True, flip=True)
    V, F = len(views), 17
    starts = [0, 1]
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(V, n, 8, S, S, generator=g) * 3).to(device)
    prob = torch.empty(F, H, W, dtype=torch.int16, device=device)
    us = timed(lambda: ops.frame_probs(logits, views, starts, F, H, W, prob=prob))
    frames = sum(1 for s in starts for k in range(8) if s + 2 * k < F)
    cover = np.zeros((H, W), np.int64)
    for h0, w0, _fl in views:
        cover[h0:h0 + S, w0:w0 + S] += 1
    nbytes = frames * (int(cover.sum()) * 4 + H * W * 2)
    return dict(us_per_call=us, frames=frames, views=V, clips=n, S=S, frame_hw=[H, W], algorithmic_bytes=nbytes, gb_per_s=nbytes / us * 1e-3,
                fraction_of_8tbs_roof=nbytes / us * 1e-3 / ROOF_GBS,
                note="the logits are re-read by every launch and stay cache-resident: not an HBM rate")


def scores_alone(F=40, H=240, W=320, device="cuda"):
    """The planted blob masks of tools/bench_detect_instances.py (a few discs per frame, some specks), their map of ranks from
    pc_frame_instances, a random probability map."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            m[f] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        m[f][rng.integers(0, H, 12), rng.integers(0, W, 12)] = 1
    mask = torch.from_numpy(m).to(device)
    _inst, imap = ops.frame_instances(mask, conn=CONN, min_area=MIN_AREA, K=K)
    prob = torch.from_numpy(rng.integers(32768, 65536, (F, H, W)).astype(np.uint16).view(np.int16)).to(device)
    out = torch.empty(F, ops.SCORE_WORDS * (K + 1), dtype=torch.int32, device=device)
    us = timed(lambda: ops.instance_scores(imap, prob, K, out=out))
    fg = int(m.sum())
    nbytes = F * H * W + 2 * fg + out.numel() * 4
    _sums, npix = ops.decode_instance_scores(out, K)
    return dict(us_per_call=us, frames=F, frame_hw=[H, W], K=K, foreground_pixels=fg, every_foreground_pixel_counted=bool(int(npix.sum()) == fg),
                algorithmic_bytes=nbytes, gb_per_s=nbytes / us * 1e-3, fraction_of_8tbs_roof=nbytes / us * 1e-3 / ROOF_GBS, bound="latency",
                note="one 256-thread block per frame, F blocks on 256 CUs; the maps are re-read by every launch and stay cache-resident: not an HBM rate")


def same_fields(a, b):
    names = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")
    return a.label == b.label and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in names) and \
        np.array_equal(a.frame_scores.view(np.int32), b.frame_scores.view(np.int32)) and torch.equal(a.masks, b.masks) and torch.equal(a.imap, b.imap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instance_scores needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    videos = [v[0] for v in synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))]
    state = synthetic.init_state(47, 24)
    kw = dict(bs=14, hw=hw, state=state, capacity=1024, instances=K, min_area=MIN_AREA, conn=CONN, instance_maps=True)
    parent = detect.DetectEngine(**kw)
    feature = detect.DetectEngine(instance_scores=True, **kw)
    configs = {}
    for pack in (True, False):
        tag = "pack" if pack else "nopack"
        configs["parent_" + tag] = lambda pack=pack: engine_pass(parent, videos, pack)
        configs["scores_" + tag] = lambda pack=pack: engine_pass(feature, videos, pack)
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = parent.n_clips
    same = all(same_fields(p, s) for t in ("pack", "nopack") for p, s in zip(results["parent_" + t], results["scores_" + t]))
    dets = results["scores_nopack"]
    frames = sum(d.counts.size for d in dets)
    over = sum(int((d.inst_flags & 1).sum()) for d in dets)
    spread = [float(d.inst_scores[f, :int(d.inst_kept[f])].max() - d.inst_scores[f, :int(d.inst_kept[f])].min())
              for d in dets for f in range(d.counts.size) if d.inst_kept[f] > 1]
    times = {k: [] for k in configs}
    for _ in range(a.passes):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    report = {
        "metric": "detection clips/sec from decoded uint8 video with a confidence per instance (frames %d x %d, 8x%dx%d clips, K = %d)" % (H, W, hw, hw, K),
        "value": nclips / med["scores_pack"], "unit": "clips/s", "videos": a.videos, "clips": nclips, "passes": a.passes, "frame_hw": [H, W],
        "parent": "the parent commit's (%s) path: DetectEngine(instances=%d, instance_maps=True)" % (PARENT_COMMIT, K),
        "clips_per_s": {k: nclips / v for k, v in med.items()},
        "pass_seconds_median": med, "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "scores_over_parent": {t: med["parent_" + t] / med["scores_" + t] for t in ("pack", "nopack")},
        "existing_fields_equal": bool(same), "frames": frames, "frames_over_run_cap": over,
        "frames_with_two_or_more_instances": len(spread), "median_score_spread_in_those": statistics.median(spread) if spread else None,
        "frame_probs": probs_alone(), "instance_scores": scores_alone(),
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
