#!/usr/bin/env python3
"""Evaluation from decoded uint8 video on one MI355X: evalstep.EvalEngine against the path it replaces.

Both paths get the same synthetic videos (synthetic.make_eval_videos_u8: uint8 frames of 240 x 256, uint8 truth) and the same weights:
  baseline   evalmetrics.evaluate(module, videos, pack=...) through the nn.Module, its body unchanged from commit 7725176, fed what the
             reference's loader yields: the centre crop divided by 255 on the host (float64 [F,224,224,3]) and the cropped truth.  The crop
             and the division are done before the clock starts -- they are the loader's work, not the evaluation's
  engine     EvalEngine.evaluate(videos_u8, pack=...): uint8 upload, clips cut on the device, one plan, tables on the device
One warm-up pass each, then `--passes` rounds that alternate the four configurations; the median clips/s of each is reported, and the tables
of all four must be equal.  The two new HBM-bound kernels are timed alone (device events, 20 launches after 3) and reported as GB/s of
their algorithmic bytes against the 8 TB/s roof; their sources are re-read every launch and fit the Infinity Cache, so the read side of
these figures is not an HBM read.

    python tools/bench_eval_u8.py --out profiles/eval_u8_bench.json [--videos 24] [--passes 5]
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
from picons_amd import evalmetrics, evalstep, model as pmodel, ops, synthetic  # noqa: E402

BASELINE_COMMIT = "7725176"
HBM_PEAK_GBS = 8000.0
TABLES = ("frame_ious", "video_ious", "n_tot_frames", "n_vids")


def kernel_rates(hw, device="cuda"):
    """The two kernels alone -> dicts for the report."""
    out = {}
    rng = np.random.default_rng(3)
    F, H, W = 200, hw + 16, hw + 32
    h0, w0 = evalstep.centre_crop(H, W, hw)
    video = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(device)
    truth = torch.from_numpy((rng.random((F, H, W)) < 0.2).astype(np.uint8)).to(device)

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    flags = torch.empty(F, dtype=torch.int32, device=device)
    ms = timed(lambda: ops.truth_frame_flags(truth, h0, w0, hw, flags))
    nbytes = F * hw * hw + 4 * F                                       # one truth byte per crop pixel read, one int32 per frame written
    out["truth_frame_flags"] = dict(frames=F, ms=ms, algorithmic_bytes=nbytes, bound="hbm", achieved=nbytes / 1e9 / (ms * 1e-3), peak=HBM_PEAK_GBS,
                                    unit="GB/s", frac=nbytes / 1e9 / (ms * 1e-3) / HBM_PEAK_GBS)
    n = 14
    starts = [(16 * (c // 2) + c % 2) for c in range(n)]               # 7 windows x 2 phases: every frame below F
    assert max(starts) + 14 < F
    data = torch.empty(n, 8, hw, hw, 4, device=device); gt = torch.empty(n, 8, hw, hw, device=device)
    ms = timed(lambda: ops.eval_clips_from_u8(video, truth, h0, w0, hw, starts, 2, out=(data, gt)))
    nbytes = n * 8 * hw * hw * (4 + 20)                                # 3 + 1 bytes read, 16 + 4 written per pixel
    out["eval_clips_from_u8"] = dict(clips=n, ms=ms, algorithmic_bytes=nbytes, bound="hbm", achieved=nbytes / 1e9 / (ms * 1e-3), peak=HBM_PEAK_GBS,
                                     unit="GB/s", frac=nbytes / 1e9 / (ms * 1e-3) / HBM_PEAK_GBS)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--bs", type=int, default=14)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_u8 needs a GPU: nothing here is measured without one")
    hw = a.hw
    vids_u8 = synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw)
    vids_f = []
    for frames, truth, label in vids_u8:                               # what the reference's loader yields (ucf_dataloader_eval.py:96-106)
        h0, w0 = evalstep.centre_crop(frames.shape[1], frames.shape[2], hw)
        vids_f.append((frames[:, h0:h0 + hw, w0:w0 + hw] / 255., truth[:, h0:h0 + hw, w0:w0 + hw], label))
    module = pmodel.CapsNet(pt_path=None, hw=hw, init="conditioned").cuda()
    module.eval(); module.training = False
    engine = evalstep.EvalEngine(bs=a.bs, hw=hw, state=module.state_dict())

    configs = {
        "module": lambda: evalmetrics.evaluate(module, vids_f, clip_batch_size=a.bs, pack=False).result(),
        "module_packed": lambda: evalmetrics.evaluate(module, vids_f, clip_batch_size=a.bs, pack=True).result(),
        "engine": lambda: engine.evaluate(vids_u8, pack=False),
        "engine_packed": lambda: engine.evaluate(vids_u8, pack=True),
    }
    results = {k: fn() for k, fn in configs.items()}                   # warm-up: plans built, kernels loaded, page-locked buffers grown
    nclips = engine.n_clips
    same = all(np.array_equal(results[k][t], results["module"][t]) for k in configs for t in TABLES) and \
        len({results[k]["n_correct"] for k in configs}) == 1
    times = {k: [] for k in configs}
    for _ in range(a.passes):
        for k, fn in configs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                       # ends in the read-back of the tables
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    rate = {k: nclips / statistics.median(v) for k, v in times.items()}
    report = {
        "metric": "eval clips/sec from decoded uint8 video (bs=%d clips, 8x%dx%d, eval forward + f-mAP/v-mAP accumulation)" % (a.bs, hw, hw),
        "value": rate["engine"], "unit": "clips/s", "videos": a.videos, "videos_skipped": engine.n_skipped, "clips": nclips, "passes": a.passes,
        "baseline": "evalmetrics.evaluate through the nn.Module as of commit %s, fed the centre crop / 255. in float64" % BASELINE_COMMIT,
        "clips_per_s": rate,
        "pass_seconds": {k: sorted(v) for k, v in times.items()},
        "engine_over_module": rate["engine"] / rate["module"], "engine_over_module_packed": rate["engine_packed"] / rate["module_packed"],
        "same_tables": bool(same),
        "kernels": kernel_rates(hw),
        "fmAP@0.5": float(results["engine"]["fmAP"][10]),
    }
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
