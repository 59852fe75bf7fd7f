#!/usr/bin/env python3
"""Overlapping clips in time on one MI355X: what DetectEngine.set_clip_hop costs, and what it costs to get the same result without it.

The synthetic uint8 videos of synthetic.make_eval_videos_u8 with frames of 240 x 256 and the synthetic weights, as the sibling benches use
them, on the centre-crop engine (bs = 14, pack=True).  Four passes over the same videos:
  hop16      today's cut: every frame in one clip (pc_detect_frames per video segment)
  hop8       set_clip_hop(8): pc_clip_planes per video segment, pc_detect_frames_planes behind each video's last clip
  hop4       set_clip_hop(4)
  by_hand    the hop-8 result without the two entries' outputs: the same hopped engine with masks=False feeds its batches to an on_batch
             hook that adds every clip's logits into a per-video torch buffer (index_add_ in clip order) and counts the clips per frame;
             then mean, sigmoid and threshold on the device, a synchronous .cpu() of every mask, the boxes in numpy.  Its masks and boxes
             must equal the engine's (checked once, on the warm-up).  The engine's own two launches still run inside this route: its time
             is an upper bound by their cost, which `kernels_alone` gives.
One warm-up, then `--passes` rounds that alternate the four; medians; the device is synchronised around every pass.  Then pc_clip_planes (the
eight clips of one 40-frame video at hop 8 in one launch) and pc_detect_frames_planes (its 40 frames in one range) alone, 20 calls after 3
with device events around all 20: microseconds, and GB/s of ALGORITHMIC bytes computed from the shapes against the 8 TB/s roof.  Their
inputs are re-read call after call and fit the 256 MB last-level cache: not an HBM rate.  Nothing is gated.

    python tools/bench_detect_hop.py --out profiles/detect_hop_bench.json [--videos 24] [--passes 5]
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
FS = 2


def run_pass(de, videos, hop):
    de.set_clip_hop(hop)
    de.begin(True)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def by_hand_route(de, videos, hop):
    """-> (masks uint8 [F,H,W] on the host, boxes int [F,4]) per video."""
    hw = de.hw
    sums, cnts = {}, {}

    def hook(m, logits, scores):
        slot = 0
        for rec, first, n in de.batch:
            key = id(rec)
            if key not in sums:
                sums[key] = torch.zeros(rec.F, hw, hw, device=de.dev)
                cnts[key] = torch.zeros(rec.F, device=de.dev)
            for c in range(n):
                idx = rec.starts[first + c] + FS * torch.arange(8, device=de.dev)
                ok = idx < rec.F
                sums[key].index_add_(0, idx[ok], logits[slot + c, 0][ok])
                cnts[key].index_add_(0, idx[ok], torch.ones(int(ok.sum()), device=de.dev))
            slot += n
    de.on_batch = hook
    run_pass(de, videos, hop)
    de.on_batch = None
    out = []
    for rec in de.videos:
        mean = sums[id(rec)] / cnts[id(rec)][:, None, None]
        m = torch.zeros(rec.F, rec.H, rec.W, dtype=torch.uint8, device=de.dev)
        m[:, rec.h0:rec.h0 + hw, rec.w0:rec.w0 + hw] = torch.sigmoid(mean) >= 0.5
        m = m.cpu().numpy()
        boxes = np.zeros((rec.F, 4), np.int32)
        for f in range(rec.F):
            ys, xs = np.nonzero(m[f])
            if ys.size:
                boxes[f] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1)
        out.append((m, boxes))
    return out


def measure(de, hand, videos, passes):
    routes = (("hop16", lambda: run_pass(de, videos, 16)), ("hop8", lambda: run_pass(de, videos, 8)), ("hop4", lambda: run_pass(de, videos, 4)),
              ("by_hand", lambda: by_hand_route(hand, videos, 8)))
    clips = {}
    for k, fn in routes:                                              # warm-up
        first = fn()
        clips[k] = (hand if k == "by_hand" else de).n_clips
        if k == "hop8":
            want = [(d.masks.cpu().numpy(), d.boxes) for d in first]
        if k == "by_hand":
            same_masks = all(np.array_equal(a[0], b[0]) for a, b in zip(want, first))
            same_boxes = all(np.array_equal(a[1], b[1]) for a, b in zip(want, first))
    if not (same_masks and same_boxes):
        raise SystemExit("bench_detect_hop: the by-hand hop-8 result differs from the engine's (masks equal: %s, boxes equal: %s)" % (same_masks, same_boxes))
    torch.cuda.synchronize()
    times = {k: [] for k, _fn in routes}
    for _ in range(passes):
        for k, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    per_clip16 = med["hop16"] / clips["hop16"]
    return dict(frames=sum(v.shape[0] for v in videos), clips=clips, seconds_median=med, seconds={k: sorted(v) for k, v in times.items()},
                clips_per_s={k: clips[k] / med[k] for k in med}, by_hand_masks_equal=same_masks, by_hand_boxes_equal=same_boxes,
                by_hand_over_hop8=med["by_hand"] / med["hop8"],
                predicted_from_hop16_cost_per_clip={k: per_clip16 * clips[k] for k in ("hop8", "hop4")},
                measured_over_predicted={k: med[k] / (per_clip16 * clips[k]) for k in ("hop8", "hop4")},
                host_waits={"hop16": 1, "hop8": 1, "hop4": 1, "by_hand": 1 + len(videos)},
                mask_bytes_to_host={"hop16": 0, "hop8": 0, "hop4": 0, "by_hand": sum(int(np.prod(v.shape[:3])) for v in videos)})


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


def kernels_alone(hw, H, W, hop):
    F = 40
    starts = detect.clip_starts_hop(F, FS, hop)
    n, views = len(starts), [evalstep.centre_crop(H, W, hw) + (0,)]
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(1, n, 8, hw, hw, generator=g) * 3).cuda()
    planes = torch.empty(ops.clip_planes_bytes(F, H, W, FS, hop), dtype=torch.uint8, device="cuda")
    mask = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    prob = torch.empty(F, H, W, dtype=torch.int16, device="cuda")
    rec = torch.empty(F, 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.detect_frames_planes_ws_bytes(F, H, W), dtype=torch.uint8, device="cuda")
    us_planes = timed(lambda: ops.clip_planes(logits, views, starts, F, H, W, FS, hop, planes=planes, cover=True))
    frames = lambda p: ops.detect_frames_planes(planes, F, H, W, H, W, 1, FS, hop, mask=mask, prob=p, rec=rec, ws=ws)
    us_frames, us_frames_noprob = timed(lambda: frames(prob)), timed(lambda: frames(None))
    ps = (H * W + 3) // 4 * 4
    real = sum(1 for s in starts for k in range(8) if s + FS * k < F)                   # (clip, frame) pairs below F
    b_planes = real * (hw * hw * 4 + ps * 4) + ps                                        # every logit once, every plane pixel written, the cover
    b_frames = real * H * W * 4 + F * H * W * (1 + 1 + 2)                                # every filled plane once, cover, mask, probability
    out = dict(hop=hop, frames=F, clips=n, clip_frames=real, frame_hw=[H, W], planes_bytes=planes.numel(), workspace_bytes=ws.numel(),
               positive_fraction=float(mask.float().mean()),
               note="planes (%.0f MB) and logits (%.0f MB) are re-read by every call and fit the 256 MB last-level cache: cache-resident, not an HBM rate"
                    % (planes.numel() * 1e-6, logits.numel() * 4e-6))
    for name, us, b, launches in (("pc_clip_planes", us_planes, b_planes, 1), ("pc_detect_frames_planes", us_frames, b_frames, 2)):
        frac = b / us * 1e-3 / ROOF_GBS
        out[name] = dict(us_per_call=us, launches=launches, algorithmic_bytes=b, gb_per_s=b / us * 1e-3, fraction_of_8tbs_roof=frac,
                         bound="launch latency and occupancy of a small grid, not HBM" if frac < 0.25 else "memory traffic")
    out["pc_detect_frames_planes"]["us_per_call_without_prob"] = us_frames_noprob
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_hop needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 32
    made = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos = [v[0] for v in made]
    state = synthetic.init_state(47, 24)
    de = detect.DetectEngine(hw=hw, state=state, capacity=4096, bs=14, pack=True)
    hand = detect.DetectEngine(hw=hw, state=state, capacity=4096, bs=14, pack=True, masks=False)
    report = {"metric": "seconds for a detection pass over %d videos of %d x %d at clip hop 16 (today's cut), 8 and 4, centre crop, pack=True" % (a.videos, H, W),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W], "f_skip": FS, "gated": False,
              "by_hand": "the hop-8 masks and boxes from on_batch: index_add_ of every clip's logits into a per-video buffer, mean, sigmoid, threshold on the "
                         "device, .cpu() of every mask, boxes in numpy"}
    report.update(measure(de, hand, videos, a.passes))
    report["value"] = report["seconds_median"]["hop8"]
    report["kernels_alone_hop8"] = kernels_alone(hw, H, W, 8)
    report["kernels_alone_hop4"] = kernels_alone(hw, H, W, 4)
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
