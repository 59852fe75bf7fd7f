#!/usr/bin/env python3
"""Detection on a resized working frame with results at native size on one MI355X: DetectEngine.set_working_frame against the route a caller
has without it.

The synthetic uint8 videos of synthetic.make_eval_videos_u8 with frames of 240 x 320 and the synthetic weights, as the sibling benches use
them, at the working frame 256 x 256 "area" (the JHMDB loader's), on two engines: the centre crop (bs = 14) and tile + flip (8 views a
clip, bs = 16).  Three passes over the same videos, masks at the video's own 240 x 320 at the end of each:
  scaled     engine.set_working_frame((256, 256), "area"): per video one pc_resize_u8, the views cut from the working video, one
             pc_detect_frames_scaled per video segment; masks [F, 240, 320] on the device, one host wait (results())
  by_hand    what a caller does today: every video to the device and through ops.resize_u8 by hand, a pass at working size, a synchronous
             .cpu() of every working-size mask and a host upsample to native (torch.nn.functional.interpolate, bilinear on the 0 / 1 mask,
             >= 0.5) -- masks on the HOST, resampled from the thresholded mask and not from the logits: not the same pixels
  unscaled   the engine at the videos' own scale (no working frame): what the feature costs beside it
One warm-up, then `--passes` rounds that alternate the three; medians.  Then pc_detect_frames_scaled alone on one 40-frame video (its six
clips in one launch), 20 calls after 3 with device events around all 20, for the centre crop and for tile + flip: microseconds, and GB/s of
ALGORITHMIC bytes (every logit of a real frame once, the plane written and read once, mask and probability written) against the 8 TB/s
roof.  The logits (77 MB for tile + flip) are re-read call after call and fit the 256 MB last-level cache: not an HBM rate.  Nothing is gated.

    python tools/bench_detect_scaled.py --out profiles/detect_scaled_bench.json [--videos 24] [--passes 5]
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
WORK, INTERP = (256, 256), "area"


def run_pass(de, videos):
    de.begin(True)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def scaled_route(de, videos):
    de.set_working_frame(WORK, INTERP)
    dets = run_pass(de, videos)
    return [d.masks for d in dets]


def unscaled_route(de, videos):
    de.set_working_frame(None)
    dets = run_pass(de, videos)
    return [d.masks for d in dets]


def by_hand_route(de, videos):
    de.set_working_frame(None)
    dev = [ops.resize_u8(torch.from_numpy(v).to(de.dev), WORK[0], WORK[1], detect.INTERPOLATIONS[INTERP]) for v in videos]
    dets = run_pass(de, dev)
    out = []
    for v, d in zip(videos, dets):
        m = d.masks.cpu().float()[:, None]
        out.append((torch.nn.functional.interpolate(m, size=v.shape[1:3], mode="bilinear", align_corners=False)[:, 0] >= 0.5).to(torch.uint8))
    return out


def measure(de, videos, passes):
    routes = (("scaled", scaled_route), ("by_hand", by_hand_route), ("unscaled", unscaled_route))
    first = {k: fn(de, videos) for k, fn in routes}                  # warm-up
    torch.cuda.synchronize()
    a = torch.cat([m.reshape(-1) for m in first["scaled"]]).cpu()
    b = torch.cat([m.reshape(-1) for m in first["by_hand"]])
    times = {k: [] for k, _fn in routes}
    for _ in range(passes):
        for k, fn in routes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(de, videos)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    frames = sum(v.shape[0] for v in videos)
    native = sum(v.shape[0] * v.shape[1] * v.shape[2] for v in videos)
    return dict(frames=frames, native_pixels=native, seconds_median=med, seconds={k: sorted(v) for k, v in times.items()},
                scaled_over_by_hand=med["by_hand"] / med["scaled"], scaled_over_unscaled=med["scaled"] / med["unscaled"],
                mask_bytes_to_host={"scaled": 0, "by_hand": frames * WORK[0] * WORK[1], "unscaled": 0},
                host_waits={"scaled": 1, "by_hand": 1 + len(videos), "unscaled": 1},
                positive_fraction={"scaled": float(a.float().mean()), "by_hand": float(b.float().mean())},
                pixels_that_differ_scaled_vs_by_hand=float((a != b).float().mean()))


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


def kernel_alone(hw, H, W, views, what):
    F, (Hs, Ws) = 40, WORK
    starts = evalstep.clip_starts(F, np.ones(F))
    n, V = len(starts), len(views)
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(V, n, 8, hw, hw, generator=g) * 3).cuda()
    mask = torch.empty(F, H, W, dtype=torch.uint8, device="cuda")
    prob = torch.empty(F, H, W, dtype=torch.int16, device="cuda")
    rec = torch.empty(F, 8, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W), dtype=torch.uint8, device="cuda")
    call = lambda p: ops.detect_frames_scaled(logits, views, starts, F, H, W, Hs, Ws, mask=mask, prob=p, rec=rec, ws=ws)
    us, us_noprob = timed(lambda: call(prob)), timed(lambda: call(None))
    b = F * (V * hw * hw * 4 + 2 * 5 * Hs * Ws + 3 * H * W)
    return dict(views=what, V=V, frames=F, clips=n, work_hw=[Hs, Ws], native_hw=[H, W], launches=3, us_per_call=us, us_per_call_without_prob=us_noprob,
                algorithmic_bytes=b, gb_per_s=b / us * 1e-3, fraction_of_8tbs_roof=b / us * 1e-3 / ROOF_GBS, workspace_bytes=ws.numel(),
                positive_fraction=float(mask.float().mean()),
                note="the logits (%.0f MB) are re-read by every call and fit the 256 MB last-level cache: cache-resident, not an HBM rate" % (logits.numel() * 4e-6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_scaled needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    made = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))
    videos = [v[0] for v in made]
    state = synthetic.init_state(47, 24)
    report = {"metric": "seconds for a detection pass at working frame %d x %d (%s) with masks at the native %d x %d (%d videos, centre crop)"
                        % (WORK + (INTERP, H, W, a.videos)),
              "unit": "s", "videos": a.videos, "passes": a.passes, "frame_hw": [H, W], "work_hw": list(WORK), "interpolation": INTERP,
              "scaled": "set_working_frame: resize, cut, forward, pc_detect_frames_scaled; native masks on the device",
              "by_hand": "ops.resize_u8 by hand, a pass at working size, .cpu() of every working-size mask, host bilinear upsample of the 0 / 1 mask",
              "unscaled": "the engine at the videos' own scale", "gated": False}
    for name, kw in (("centre_crop", dict(bs=14)), ("tile_flip", dict(bs=16, tile=True, flip=True))):
        de = detect.DetectEngine(hw=hw, state=state, capacity=2048, **kw)
        report[name] = dict(measure(de, videos, a.passes), views=len(detect.make_views(WORK[0], WORK[1], hw, kw.get("tile", False), kw.get("flip", False))),
                            clips=de.n_clips)
        del de
    report["value"] = report["centre_crop"]["seconds_median"]["scaled"]
    report["kernel_alone_centre"] = kernel_alone(hw, H, W, [evalstep.centre_crop(WORK[0], WORK[1], hw) + (0,)], "the centre crop of the working frame")
    report["kernel_alone_tile_flip"] = kernel_alone(hw, H, W, detect.make_views(WORK[0], WORK[1], hw, True, True), "tile + flip of the working frame")
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
