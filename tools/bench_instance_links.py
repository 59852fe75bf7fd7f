#!/usr/bin/env python3
"""Mask overlaps between frames on one MI355X: detect.DetectEngine(instance_links=1) against the engine without it, and against what a caller
who wants mask-overlap linking does without it.

All configurations get the same synthetic uint8 videos (synthetic.make_eval_videos_u8 with frames of 240 x 320; the truth is not used) and
the same weights, at pack=True and pack=False:
  parent   the path of the parent commit 653f0ab: DetectEngine(instances=8, instance_maps=True)
  links    the same engine with instance_links=1: one pc_instance_overlaps launch per video behind pc_frame_instances, the records in the
           same copy
  host     the HOST BASELINE a caller runs today: the parent's pass, then a device-to-host copy of every video's map of ranks and the numpy
           histogram per pair of consecutive frames
One warm-up pass per configuration, then `--passes` rounds that alternate them; medians.  The tool checks that every existing field of
`links` equals the parent's and that its overlaps equal the host's.
Then the kernel alone, 20 launches after 3 with device events around all 20: pc_instance_overlaps on the maps of planted blob masks (F = 40,
240 x 320, K = 8, the masks of tools/bench_detect_instances.py) at L = 1 and L = 4.  Given in microseconds and as GB/s of ALGORITHMIC bytes
(every map byte of the first frame of a pair, the partner's bytes under its foreground, the record) against the 8 TB/s roof -- but the maps
are re-read launch after launch and are cache-resident, as they are in the engine, where pc_frame_instances has just written them: the figure
is not an HBM rate, and with F * L blocks on 256 CUs the launch is latency-bound like its siblings.  Nothing is gated.

    python tools/bench_instance_links.py --out profiles/instance_links_bench.json [--videos 24] [--passes 5]
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

PARENT_COMMIT = "653f0ab"
K, CONN, MIN_AREA = 8, 8, 1
ROOF_GBS = 8000.0


def host_overlaps(imap, K, L):
    """The numpy histogram: imap uint8 [F,H,W] -> int32 [F, L, K + 1, K + 1]."""
    F = imap.shape[0]
    v = imap.reshape(F, -1).astype(np.int64)
    slot = np.where(v == 0, -1, np.where(v <= K, v - 1, K))
    out = np.zeros((F, L, K + 1, K + 1), np.int32)
    for f in range(F):
        for lag in range(L):
            g = f + lag + 1
            if g < F:
                both = (slot[f] >= 0) & (slot[g] >= 0)
                out[f, lag] = np.bincount(slot[f][both] * (K + 1) + slot[g][both], minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    return out


def engine_pass(de, videos, pack):
    de.begin(pack)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def host_pass(de, videos, pack):
    dets = engine_pass(de, videos, pack)
    return dets, [host_overlaps(d.imap.cpu().numpy(), K, 1) for d in dets]


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


def blob_maps(F=40, H=240, W=320, device="cuda"):
    """The planted blob masks of tools/bench_detect_instances.py (a few discs per frame, some specks) and their map of ranks."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            m[f] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        m[f][rng.integers(0, H, 12), rng.integers(0, W, 12)] = 1
    _inst, imap = ops.frame_instances(torch.from_numpy(m).to(device), conn=CONN, min_area=MIN_AREA, K=K)
    return imap


def overlaps_alone(imap, L):
    F, H, W = (int(v) for v in imap.shape)
    out = torch.empty(F, L, K + 1, K + 1, dtype=torch.int32, device=imap.device)
    us = timed(lambda: ops.instance_overlaps(imap, K, L, out=out))
    host = imap.cpu().numpy()
    want = host_overlaps(host, K, L)
    fg = (host != 0).reshape(F, -1)
    pairs = [(f, f + lag + 1) for f in range(F) for lag in range(L) if f + lag + 1 < F]
    nbytes = sum(H * W + int(fg[f].sum()) for f, _g in pairs) + out.numel() * 4
    return dict(us_per_call=us, frames=F, lags=L, blocks=F * L, pairs=len(pairs), frame_hw=[H, W], K=K, foreground_pixels=int(fg.sum()),
                shared_pixels=int(want.sum()), equal_to_host_histogram=bool(np.array_equal(out.cpu().numpy(), want)),
                algorithmic_bytes=nbytes, gb_per_s=nbytes / us * 1e-3, fraction_of_8tbs_roof=nbytes / us * 1e-3 / ROOF_GBS, bound="latency",
                note="one 256-thread block per (frame, lag), F * L blocks on 256 CUs; the maps are re-read by every launch and stay cache-resident: not an HBM rate")


def same_fields(a, b):
    names = ("counts", "boxes", "inst_n", "inst_kept", "inst_flags", "inst_areas", "inst_boxes", "inst_first")
    return a.label == b.label and all(np.array_equal(getattr(a, k), getattr(b, k)) for k in names) and \
        np.array_equal(a.frame_scores.view(np.int32), b.frame_scores.view(np.int32)) and \
        np.array_equal(a.class_scores.view(np.int32), b.class_scores.view(np.int32)) and torch.equal(a.masks, b.masks) and torch.equal(a.imap, b.imap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instance_links needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    videos = [v[0] for v in synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))]
    state = synthetic.init_state(47, 24)
    kw = dict(bs=14, hw=hw, state=state, capacity=1024, instances=K, min_area=MIN_AREA, conn=CONN, instance_maps=True)
    parent = detect.DetectEngine(**kw)
    feature = detect.DetectEngine(instance_links=1, **kw)
    configs = {}
    for pack in (True, False):
        tag = "pack" if pack else "nopack"
        configs["parent_" + tag] = lambda pack=pack: engine_pass(parent, videos, pack)
        configs["links_" + tag] = lambda pack=pack: engine_pass(feature, videos, pack)
        configs["host_" + tag] = lambda pack=pack: host_pass(parent, videos, pack)
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = parent.n_clips
    same = all(same_fields(p, s) for t in ("pack", "nopack") for p, s in zip(results["parent_" + t], results["links_" + t]))
    equal = all(np.array_equal(d.inst_overlaps, h) for t in ("pack", "nopack") for d, h in zip(results["links_" + t], results["host_" + t][1]))
    dets = results["links_nopack"]
    frames = sum(d.counts.size for d in dets)
    over = sum(int((d.inst_flags & 1).sum()) for d in dets)
    by_box = sum(len(d.instance_tubes()) for d in dets)
    by_mask = sum(len(d.instance_tubes(link="mask")) for d in dets)
    times = {k: [] for k in configs}
    for _ in range(a.passes):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    imap = blob_maps()
    report = {
        "metric": "detection clips/sec from decoded uint8 video with mask overlaps between consecutive frames (frames %d x %d, 8x%dx%d clips, K = %d, L = 1)"
                  % (H, W, hw, hw, K),
        "value": nclips / med["links_pack"], "unit": "clips/s", "videos": a.videos, "clips": nclips, "passes": a.passes, "frame_hw": [H, W],
        "parent": "the parent commit's (%s) path: DetectEngine(instances=%d, instance_maps=True)" % (PARENT_COMMIT, K),
        "host": "the host baseline a caller runs today: the parent's pass, every imap copied to the host, the numpy histogram per pair of frames",
        "clips_per_s": {k: nclips / v for k, v in med.items()},
        "pass_seconds_median": med, "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "links_over_parent": {t: med["parent_" + t] / med["links_" + t] for t in ("pack", "nopack")},
        "links_over_host": {t: med["host_" + t] / med["links_" + t] for t in ("pack", "nopack")},
        "existing_fields_equal": bool(same), "overlaps_equal_to_host_histogram": bool(equal), "frames": frames, "frames_over_run_cap": over,
        "instance_tubes_by_box": by_box, "instance_tubes_by_mask": by_mask,
        "instance_overlaps_L1": overlaps_alone(imap, 1), "instance_overlaps_L4": overlaps_alone(imap, 4),
        "gated": False,
    }
    assert same and equal, "the engine with instance_links differs from the parent's fields or from the host histogram"
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
