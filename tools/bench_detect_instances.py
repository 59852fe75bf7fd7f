#!/usr/bin/env python3
"""Per-frame instances on one MI355X: detect.DetectEngine(instances=8) against the engine without them and against what a user does today
for the same answer.

Every configuration gets the same synthetic uint8 videos (synthetic.make_eval_videos_u8 with frames of 240 x 320; the truth is not used) and
the same weights, at pack=True and pack=False:
  parent     the path of the parent commit fdb9392: DetectEngine(instances=0) -- masks, one box per frame
  instances  DetectEngine(instances=8): one pc_frame_instances launch per video behind its last clip, the records in the same copy
  host       the baseline, what a user does today: the parent path, then a device-to-host copy of every mask and host labelling
             (scipy.ndimage.label + find_objects if scipy is there, else the numpy restatement of tests/instances_ref.py), ranked on the host
One warm-up pass per configuration, then `--passes` rounds that alternate them; medians.  The tool checks that the host baseline's areas and
boxes equal the engine's.  Then pc_frame_instances alone: F = 40 frames of 240 x 320, K = 8, 20 launches after 3, device events around all 20,
microseconds per call on planted blob masks (a few discs and specks per frame, all within the run cap; the host labels the same frames and
the records are compared) -- a latency-bound kernel (F blocks on 256 CUs, a 77 KB frame stays in L2), so no fraction of a roof is given.  Nothing
is gated.

    python tools/bench_detect_instances.py --out profiles/detect_instances_bench.json [--videos 24] [--passes 5]
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

PARENT_COMMIT = "fdb9392"
K, CONN, MIN_AREA = 8, 8, 1

try:
    from scipy import ndimage as ndi
    LABELLER = "scipy.ndimage.label + find_objects"
except ImportError:
    ndi = None
    LABELLER = "tests/instances_ref.py (numpy union-find)"


def engine_pass(de, videos, pack):
    de.begin(pack)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def host_label(masks):
    """uint8 [F,H,W] on the host -> (areas [F,K], boxes [F,K,4]) ranked by area descending, first pixel ascending."""
    F, H, W = masks.shape
    areas, boxes = np.zeros((F, K), np.int32), np.zeros((F, K, 4), np.int32)
    for f in range(F):
        if ndi is not None:
            lab, n = ndi.label(masks[f], structure=np.ones((3, 3), int))
            if n == 0:
                continue
            ar = np.bincount(lab.ravel(), minlength=n + 1)[1:]
            flat = lab.ravel()
            first = np.full(n + 1, H * W, np.int64)
            idx = np.flatnonzero(flat)
            np.minimum.at(first, flat[idx], idx)
            order = sorted(range(n), key=lambda i: (-int(ar[i]), int(first[i + 1])))[:K]
            sl = ndi.find_objects(lab)
            for r, i in enumerate(order):
                areas[f, r] = ar[i]
                boxes[f, r] = (sl[i][1].start, sl[i][0].start, sl[i][1].stop, sl[i][0].stop)
        else:
            from tests import instances_ref
            rec, _imap, _runs = instances_ref.frame_instances(masks[f], CONN, MIN_AREA, K, max_runs=1 << 30)
            slots = rec[4:].reshape(K, 6)
            areas[f], boxes[f] = slots[:, 0], slots[:, 1:5]
    return areas, boxes


def host_pass(de, videos, pack):
    return [host_label(d.masks.cpu().numpy()) for d in engine_pass(de, videos, pack)]


def kernel_alone(F=40, H=240, W=320, device="cuda"):
    """Blob masks like a trained detector's (a few discs per frame, some specks) -> microseconds per pc_frame_instances call, and the host's
    time for the same frames with its records compared."""
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            m[f] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        m[f][rng.integers(0, H, 12), rng.integers(0, W, 12)] = 1
    mask = torch.from_numpy(m).to(device)
    inst = torch.empty(F, ops.INST_HDR + K * ops.INST_WORDS, dtype=torch.int32, device=device)
    imap = torch.empty(F, H, W, dtype=torch.uint8, device=device)
    out = {}
    for name, im in (("records_only", None), ("with_imap", imap)):
        fn = lambda: ops.frame_instances(mask, conn=CONN, min_area=MIN_AREA, K=K, inst=inst, imap=im, want_imap=False)
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = dict(us_per_call=e0.elapsed_time(e1) / 20 * 1e3)
    _n, _kept, runs, flags, areas, boxes, _first = ops.decode_instances(inst, K)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_areas, host_boxes = host_label(mask.cpu().numpy())            # the same frames the way a user labels them today: copy, then the host
    out["host_copy_and_label_us"] = (time.perf_counter() - t0) * 1e6
    out["same_areas_and_boxes_as_host"] = bool(not flags.any() and np.array_equal(areas, host_areas) and np.array_equal(boxes, host_boxes))
    out.update(frames=F, frame_hw=[H, W], K=K, conn=CONN, runs_per_frame_max=int(runs.max()), bound="latency",
               note="one 256-thread block per frame, F blocks on 256 CUs; a frame is %d KB and stays in L2" % (H * W // 1000))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_instances needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    videos = [v[0] for v in synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))]
    state = synthetic.init_state(47, 24)
    parent = detect.DetectEngine(bs=14, hw=hw, state=state, capacity=1024)
    feature = detect.DetectEngine(bs=14, hw=hw, state=state, capacity=1024, instances=K, min_area=MIN_AREA, conn=CONN)
    configs = {}
    for pack in (True, False):
        tag = "pack" if pack else "nopack"
        configs["parent_" + tag] = lambda pack=pack: engine_pass(parent, videos, pack)
        configs["instances_" + tag] = lambda pack=pack: engine_pass(feature, videos, pack)
        configs["host_" + tag] = lambda pack=pack: host_pass(parent, videos, pack)
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = parent.n_clips
    # the host baseline labels every frame; the engine falls back on a frame over the run cap: compare where it did not
    same, over, frames = True, 0, 0
    for d, (areas, boxes) in zip(results["instances_nopack"], results["host_nopack"]):
        ok = (d.inst_flags & 1) == 0
        over += int((~ok).sum()); frames += ok.size
        same = same and np.array_equal(d.inst_areas[ok], areas[ok]) and np.array_equal(d.inst_boxes[ok], boxes[ok])
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
        "metric": "detection clips/sec from decoded uint8 video with per-frame instances (frames %d x %d, 8x%dx%d clips, K = %d, conn %d)" % (H, W, hw, hw, K, CONN),
        "value": nclips / med["instances_pack"], "unit": "clips/s", "videos": a.videos, "clips": nclips, "passes": a.passes, "frame_hw": [H, W],
        "parent": "the parent commit's (%s) path: DetectEngine(instances=0)" % PARENT_COMMIT,
        "baseline": "host: what a user does today -- the parent path, a device-to-host copy of every mask, %s on the host" % LABELLER,
        "clips_per_s": {k: nclips / v for k, v in med.items()},
        "pass_seconds_median": med, "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "instances_over_parent": {t: med["parent_" + t] / med["instances_" + t] for t in ("pack", "nopack")},
        "instances_over_host": {t: med["host_" + t] / med["instances_" + t] for t in ("pack", "nopack")},
        "same_areas_and_boxes_as_host": bool(same), "frames": frames, "frames_over_run_cap": over,
        "instances_kept": sum(int(d.inst_kept.sum()) for d in results["instances_nopack"]),
        "kernel": kernel_alone(),
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
