#!/usr/bin/env python3
"""Masks and maps of ranks leaving the device as row runs on one MI355X: detect.DetectEngine.mask_runs against the export a caller does
without it.

The same synthetic uint8 videos (synthetic.make_eval_videos_u8 with frames of 240 x 320; the truth is not used) and weights as
tools/bench_instance_links.py, one engine DetectEngine(instances=8, instance_maps=True), two kinds of pixels:
  blobs    after the pass every video's mask is replaced by planted blob masks (three discs and twelve specks per frame, the masks of
           tools/bench_detect_instances.py) and its map of ranks made again from them: what a trained model's output looks like
  noise    the masks the synthetic weights give themselves: foreground density near 0.5, no structure -- the worst case for runs
and two exports of the finished pass, both ending with the pixels on the host:
  dense    today's: a synchronous .cpu() of every video's mask followed by np.packbits, and a .cpu() of every map of ranks
  runs     engine.mask_runs("masks") and engine.mask_runs("imap"): two host waits each, however many videos
One warm-up, then `--passes` rounds that alternate the two; medians, next to the median time of the pass itself.  The tool asserts that
MaskRuns.dense() equals the arrays of the dense export, byte for byte.  bytes_to_host is what crosses to the host (dense: F * H * W per map;
runs: 8 per run and 4 per frame offset), bytes_kept what a caller then holds (packbits: F * H * W / 8 for a mask).
Then the two entries alone on the blob maps of F = 40 frames, 20 launches after 3 with device events around all 20: microseconds, and GB/s
of ALGORITHMIC bytes (every map byte once, the index, the runs) against the 8 TB/s roof -- the map is re-read launch after launch and is
cache-resident, as it is in the engine: not an HBM rate.  Nothing is gated.

    python tools/bench_mask_runs.py --out profiles/mask_runs_bench.json [--videos 24] [--passes 5]
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

K, CONN, MIN_AREA = 8, 8, 1
ROOF_GBS = 8000.0


def blob_masks(F, H, W, seed):
    """Three discs and twelve specks per frame (tools/bench_detect_instances.py)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        for _ in range(3):
            cy, cx, r = rng.integers(20, H - 20), rng.integers(20, W - 20), rng.integers(8, 40)
            m[f] |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)
        m[f][rng.integers(0, H, 12), rng.integers(0, W, 12)] = 1
    return m


def engine_pass(de, videos):
    de.begin(True)
    for frames in videos:
        de.add_video(frames)
    return de.results()


def plant_blobs(de):
    """The masks of the finished pass replaced by blob masks, the maps of ranks made again from them (in place: the engine's own tensors)."""
    for i, rec in enumerate(de.videos):
        rec.mask.copy_(torch.from_numpy(blob_masks(rec.F, rec.H, rec.W, 7 + i)).to(rec.mask.device))
        ops.frame_instances(rec.mask, conn=CONN, min_area=MIN_AREA, K=K, imap=rec.imap)
    torch.cuda.synchronize()


def export_dense(de):
    masks = [rec.mask.cpu().numpy() for rec in de.videos]
    packed = [np.packbits(m) for m in masks]
    imaps = [rec.imap.cpu().numpy() for rec in de.videos]
    return masks, packed, imaps


def export_runs(de):
    return de.mask_runs("masks"), de.mask_runs("imap")


def measure(de, passes):
    """Both exports of the engine's finished pass, alternating -> the report of one kind of pixels."""
    masks, packed, imaps = export_dense(de)                              # warm-up, and the arrays the runs must decode to
    rm, ri = export_runs(de)
    equal = all(np.array_equal(r.dense(), m) for r, m in zip(rm, masks)) and all(np.array_equal(r.dense(), m) for r, m in zip(ri, imaps))
    times = {"dense": [], "runs": []}
    for _ in range(passes):
        for k, fn in (("dense", export_dense), ("runs", export_runs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(de)
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    pixels = sum(m.size for m in masks)
    n_mask, n_imap = sum(r.runs.shape[0] for r in rm), sum(r.runs.shape[0] for r in ri)
    frames = sum(m.shape[0] for m in masks)
    return dict(frames=frames, pixels=pixels, foreground_density=sum(int((m != 0).sum()) for m in masks) / pixels,
                mask_runs=n_mask, imap_runs=n_imap, runs_per_frame={"masks": n_mask / frames, "imap": n_imap / frames},
                bytes_to_host={"dense": 2 * pixels, "runs": 8 * (n_mask + n_imap) + 4 * 2 * (frames + len(masks))},
                bytes_kept={"dense": sum(p.nbytes for p in packed) + pixels, "runs": sum(r.nbytes for r in rm) + sum(r.nbytes for r in ri)},
                bytes_per_frame={"dense_mask": pixels / frames, "packbits_mask": pixels / frames / 8, "mask_runs": 8 * n_mask / frames,
                                 "imap_runs": 8 * n_imap / frames},
                export_seconds_median=med, export_seconds={k: sorted(v) for k, v in times.items()}, runs_over_dense=med["dense"] / med["runs"],
                host_waits={"dense": 2 * len(masks), "runs": 4}, dense_equal=bool(equal))


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


def entries_alone(m, what):
    F, H, W = (int(v) for v in m.shape)
    index = ops.mask_run_index(m)
    total = int(index[-1].item())
    runs = torch.empty(total, ops.RUN_WORDS, dtype=torch.int32, device=m.device)
    us_index = timed(lambda: ops.mask_run_index(m, index=index))
    us_runs = timed(lambda: ops.mask_runs(m, index, cap=total, runs=runs))
    host = m.cpu().numpy()
    want = detect.MaskRuns.from_dense(host)
    exact = bool(np.array_equal(runs.cpu().numpy().view(np.uint32), want.runs) and np.array_equal(index.cpu().numpy()[::H], want.offsets))
    b_index, b_runs = F * H * W + 4 * (F * H + 1), F * H * W + 4 * (F * H + 1) + 8 * total
    return dict(map=what, frames=F, frame_hw=[H, W], runs=total, blocks=(F * H + 31) // 32, equal_to_host_encoder=exact,
                mask_run_index=dict(us_per_call=us_index, launches=3, algorithmic_bytes=b_index, gb_per_s=b_index / us_index * 1e-3,
                                    fraction_of_8tbs_roof=b_index / us_index * 1e-3 / ROOF_GBS),
                mask_runs=dict(us_per_call=us_runs, launches=1, algorithmic_bytes=b_runs, gb_per_s=b_runs / us_runs * 1e-3,
                               fraction_of_8tbs_roof=b_runs / us_runs * 1e-3 / ROOF_GBS),
                bound="latency", note="a 240 x 320 x 40 map is 3 MB and cache-resident, re-read by every launch: not an HBM rate; the us_per_call "
                "of mask_run_index includes the allocation of its workspace by ops.mask_run_index")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--hw", type=int, default=224)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_runs needs a GPU: nothing here is measured without one")
    hw = a.hw
    H, W = hw + 16, hw + 96
    videos = [v[0] for v in synthetic.make_eval_videos_u8(a.videos, seed=5, hw=hw, frames_hw=(H, W))]
    de = detect.DetectEngine(bs=14, hw=hw, state=synthetic.init_state(47, 24), capacity=1024, instances=K, min_area=MIN_AREA, conn=CONN,
                             instance_maps=True)
    engine_pass(de, videos)                                              # warm-up: plans built, kernels loaded, page-locked buffers grown
    pass_times = []
    for _ in range(a.passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dets = engine_pass(de, videos)
        pass_times.append(time.perf_counter() - t0)
    pass_s = statistics.median(pass_times)
    noise = measure(de, a.passes)
    counts_ok = all(np.array_equal(r.areas(), d.counts.astype(np.int64)) for r, d in zip(de.mask_runs("masks"), dets))
    plant_blobs(de)
    blobs = measure(de, a.passes)
    for rep in (noise, blobs):
        rep["pass_plus_export_seconds"] = {k: pass_s + v for k, v in rep["export_seconds_median"].items()}
    blob40 = torch.from_numpy(blob_masks(40, H, W, 7)).cuda()
    _inst, imap40 = ops.frame_instances(blob40, conn=CONN, min_area=MIN_AREA, K=K)
    report = {
        "metric": "seconds to bring the masks and maps of ranks of a finished detection pass to the host as row runs (blob masks, %d videos, frames %d x %d)"
                  % (a.videos, H, W),
        "value": blobs["export_seconds_median"]["runs"], "unit": "s", "videos": a.videos, "clips": de.n_clips, "passes": a.passes, "frame_hw": [H, W],
        "pass_seconds_median": pass_s, "pass_seconds": sorted(pass_times),
        "dense": "today's export: .cpu() of every mask + np.packbits, .cpu() of every imap",
        "runs": "engine.mask_runs(\"masks\") and engine.mask_runs(\"imap\")",
        "blobs": blobs, "noise": noise, "areas_equal_counts_on_noise": bool(counts_ok),
        "entries_alone_mask": entries_alone(blob40, "blob masks, value 1"), "entries_alone_imap": entries_alone(imap40, "their map of ranks"),
        "gated": False,
    }
    assert blobs["dense_equal"] and noise["dense_equal"] and counts_ok, "MaskRuns.dense() differs from the dense export"
    line = json.dumps(report)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
