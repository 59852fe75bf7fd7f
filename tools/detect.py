#!/usr/bin/env python3
"""Detections from decoded uint8 video on one MI355X (detect.DetectEngine): where the action is and which action it is.

Weights: a checkpoint in the reference's key layout (--ckpt, a torch.save'd state_dict), or the synthetic initial state.  Videos: .npy files
of uint8 frames [F,H,W,3] with frames at least hw x hw (ops.resize_u8 scales decoded frames on the device), or --synthetic N videos of
synthetic.make_eval_videos_u8.  One pass; one .npz with, per video i: label_i, class_scores_i [C], counts_i [F], boxes_i [F,4] (x0, y0, x1, y1,
half-open, full-frame coordinates), frame_scores_i [F], tubes_i [T,3] = (t0, t1 inclusive, score), and with --masks masks_i = np.packbits of
the uint8 masks [F,H,W] (mask_shape_i to unpack them).  --tile: the whole frame instead of its centre crop, as overlapping hw x hw tiles
whose logits are averaged per pixel; --flip: every crop also mirrored left-right, the two maps averaged (bs should be a multiple of the views
per clip, e.g. --bs 16 for the 8 views of a 240 x 320 frame with both).  tile, flip and views_i [V,3] = (h0, w0, flip) are recorded.
--instances K (implies masks on the device): per frame the K largest connected components (--conn 4 | 8) of at least --min_area pixels, as
inst_n_i [F], inst_kept_i [F], inst_flags_i [F], inst_areas_i [F,K], inst_boxes_i [F,K,4], inst_first_i [F,K] and the per-actor tubes
inst_tubes_i [T,3] = (t0, t1 inclusive, score) with inst_tube_boxes_i [sum of the tubes' lengths, 4] one tube after the other; with
--instance_maps also imap_i, the uint8 map of ranks [F,H,W] as it is (imap_shape_i).
--instance_scores (needs --instances K > 0): a confidence per instance, inst_scores_i [F,K] the mean probability over the instance's own pixels
and other_score_i [F] that over the foreground no kept instance holds; the scores of inst_tubes_i are then the means of their own instances'.
--instance_links L (1..4, needs --instances K > 0): inst_overlaps_i int32 [F, L, K + 1, K + 1], the pixels slot a of frame f shares with slot b
of frame f + l + 1, counted on the device; --link mask then links inst_tubes_i by mask IoU from them (--max-gap at most L - 1) instead of by
box IoU (--link box, the default).
--mask_runs (implies masks on the device): the masks as ROW RUNS made on the device (DetectEngine.mask_runs: two host waits for the whole
pass, a frame of a few blobs is 1-2 KB): mask_runs_i uint32 [n,2] = (row | value << 24, x0 | x1 << 16) with row = f * H + y and x1 half-open,
mask_run_offsets_i int64 [F + 1] (frame f holds the runs offsets[f] .. offsets[f + 1] - 1) and mask_shape_i; detect.MaskRuns(shape, offsets,
runs).dense() gives the uint8 masks back.  With --instance_maps also imap_runs_i / imap_run_offsets_i (value: rank + 1, or 255), and imap_i
is then not written raw.  Runs are for blob masks: a noisy mask of density 0.5 holds about W / 4 runs of 8 bytes a row, more than its bytes.
--truth t0.npy ... (one uint8 [F,H,W] or [F,H,W,1] file per video, any non-zero byte is truth) with --labels l0 ... (implies masks on the
device): the pass scored against them on the device (DetectEngine.score: one pc_map_crosstab launch per video, one host wait): f-mAP and
v-mAP at 0.2 and 0.5 and the accuracy are printed, and score_table_i int32 [F, 3, 3] (pred slot x truth slot), score_counts_i [F, 3] =
(inter, union, gt), score_label_i and the arrays of the result (score_fmAP [20], score_vmAP [20], score_frame_ious, score_video_ious,
score_n_tot_frames, score_n_vids, score_n_correct, score_accuracy) are stored.  The truth is taken on the full frame, not inside the centre
crop as evalstep.EvalEngine takes it.  With --synthetic the truth and label of synthetic.make_eval_videos_u8 are used (--score).
--truth_boxes b0.npy ... instead of --truth: one int [F,R,4] file of (x, y, w, h) boxes per video, clipped as numpy clips a slice
(evalstep.BoxTruth.from_xywh); the rect table goes to the device and pc_paint_boxes paints the map there, so F * R * 20 bytes travel instead of
F * H * W.  --actors A: slot r of a frame's boxes is actor r + 1 and the pass is scored with A actors.  --score --boxes: the synthetic truth
as boxes (synthetic.make_eval_videos_boxes).  --sweep and --recut take them as they take dense truths.
--frame_size Hs Ws [--interp area|linear|nearest]: every video is resized on the device to an Hs x Ws working frame (cv2.resize's arithmetic;
the JHMDB loader's is 256 256 area), cut and run there, and detected at its NATIVE size (DetectEngine.set_working_frame: the merged logits
resampled bilinearly to every native pixel in front of the threshold).  Everything stored stays in native coordinates but views_i, which are
crops of the working frame; work_i int32 [3] = (Hs, Ws, cv2 interpolation flag) records it.  A video smaller than hw is then taken.
--hop N: the clips of a video start every N frames instead of every 16 (DetectEngine.set_clip_hop: N a multiple of f_skip = 2 in 2..16), a
frame lies in up to 16 / N of them, and mask, box, score and probability come from the mean of their merged logits; hop_i records it.  The
class is voted over all the overlapping clips.  The effect on f-mAP / v-mAP is not measured.
--sweep [t ...] (with --truth / --labels or --score; implies DetectEngine.set_keep_probs): the pass scored at every mask threshold t in (0, 1]
(none given: 0.05, 0.10 .. 0.95) from one histogram of the kept probability map per video (DetectEngine.sweep: one pc_prob_truth_hist launch
per video, one host wait).  One line per threshold: f-mAP@0.5 and v-mAP@0.5 (the mean over the classes that hold a video, as --truth prints
them) and the pixel precision and recall over every frame of every scored video; `*` marks the first threshold with the largest printed
f-mAP@0.5.  Stored: sweep_thresholds [N], sweep_words [N], sweep_fmAP [N, 20] and sweep_vmAP [N, 20] (the evaluator's own: NaN as soon as one
class holds no video), sweep_pixel int64 [N, 3] = (tp, fp, fn).
--threshold t: the masks are cut at probability >= t, t in (0, 1], instead of at sigmoid(x) >= 0.5 (DetectEngine.set_mask_threshold: the
videos keep their probability map and one pc_prob_cut launch per video cuts it at the word ceil(t * 65535), in front of the class vote and
the instances); counts, boxes, instances, runs and score are those of that mask, frame_scores_i the means of the probability words.
--sweep [t ...] --recut: after the sweep the finished pass is cut again ON THE DEVICE at the printed best threshold (DetectEngine.recut: no
second forward, one host wait), before masks, runs, score and records are stored: everything stored is the pass at that threshold.  The
sweep is then printed in front of the score.  Without a best threshold (every f-mAP@0.5 NaN) nothing is cut again.  With either option
mask_threshold and mask_word record the threshold and its word.

    python tools/detect.py --out detections.npz [--ckpt best_model.pth] [--synthetic 4 | video.npy ...] [--masks] [--pack] [--tile] [--flip]
                           [--max-gap 0] [--min-pixels 1] [--instances K] [--min_area 1] [--conn 8] [--instance_maps] [--instance_scores]
                           [--instance_links L] [--link box|mask] [--mask_runs] [--truth t0.npy ... --labels l0 ... | --truth_boxes b0.npy ... --labels l0 ... [--actors A] | --score [--boxes]]
                           [--frame_size Hs Ws [--interp area|linear|nearest]] [--hop N] [--sweep [t ...] [--recut]] [--threshold t]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import picons_amd  # noqa: F401,E402
from picons_amd import detect, evalstep, synthetic, trainstate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("videos", nargs="*", help=".npy files of uint8 frames [F,H,W,3]")
    ap.add_argument("--out", default="detections.npz")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--synthetic", type=int, default=0, help="use N synthetic videos (the default, with 4, when no file is given)")
    ap.add_argument("--classes", type=int, default=24)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--bs", type=int, default=14)
    ap.add_argument("--masks", action="store_true")
    ap.add_argument("--pack", action="store_true")
    ap.add_argument("--tile", action="store_true", help="cover the whole frame with hw x hw tiles (detect.make_views)")
    ap.add_argument("--flip", action="store_true", help="every crop also mirrored left-right")
    ap.add_argument("--min-pixels", type=int, default=1)
    ap.add_argument("--max-gap", type=int, default=0)
    ap.add_argument("--instances", type=int, default=0, help="per frame the K largest connected components of the mask (pc_frame_instances)")
    ap.add_argument("--min_area", type=int, default=1)
    ap.add_argument("--conn", type=int, default=8, choices=(4, 8))
    ap.add_argument("--instance_maps", action="store_true", help="with --instances: also the uint8 map of ranks per frame")
    ap.add_argument("--instance_scores", action="store_true", help="with --instances: a confidence per instance and per instance tube")
    ap.add_argument("--instance_links", type=int, default=0, help="with --instances: mask overlaps between frames up to L apart (pc_instance_overlaps)")
    ap.add_argument("--link", default="box", choices=("box", "mask"), help="link the instance tubes by box IoU or, with --instance_links, by mask IoU")
    ap.add_argument("--mask_runs", action="store_true", help="the masks (with --instance_maps: and the maps of ranks) as row runs made on the device")
    ap.add_argument("--truth", nargs="+", default=None, help="one .npy of uint8 truth [F,H,W] or [F,H,W,1] per video: score the pass against them")
    ap.add_argument("--labels", nargs="+", type=int, default=None, help="with --truth: one class id per video")
    ap.add_argument("--score", action="store_true", help="with synthetic videos: score the pass against their own truth and labels")
    ap.add_argument("--truth_boxes", nargs="+", default=None, help="instead of --truth: one .npy of int boxes [F,R,4] = (x, y, w, h) per video (evalstep.BoxTruth: the table goes up, the map is painted on the device)")
    ap.add_argument("--boxes", action="store_true", help="with --score: the synthetic truth as boxes (synthetic.make_eval_videos_boxes)")
    ap.add_argument("--actors", type=int, default=None, metavar="A", help="with --truth_boxes: slot r of a frame's boxes is actor r + 1, and the pass is scored with A actors")
    ap.add_argument("--frame_size", nargs=2, type=int, default=None, metavar=("Hs", "Ws"), help="resize every video to this working frame on the device; results stay at native size")
    ap.add_argument("--interp", default="area", choices=sorted(detect.INTERPOLATIONS), help="with --frame_size: cv2.resize's interpolation")
    ap.add_argument("--hop", type=int, default=None, help="cut overlapping clips that start every N frames and average the clips that hold a frame (a multiple of 2 in 2..16; 16: today's cut)")
    ap.add_argument("--sweep", nargs="*", type=float, default=None, metavar="t", help="with --truth/--labels or --score: f-mAP / v-mAP and pixel precision / recall at every mask threshold t (default 0.05 .. 0.95) from the kept probability map")
    ap.add_argument("--threshold", type=float, default=None, metavar="t", help="cut the masks at probability >= t in (0, 1] instead of at sigmoid(x) >= 0.5 (DetectEngine.set_mask_threshold)")
    ap.add_argument("--recut", action="store_true", help="with --sweep: cut the finished pass again on the device at the best threshold of the sweep before anything is stored (DetectEngine.recut)")
    a = ap.parse_args()
    if (a.truth is None and a.truth_boxes is None) != (a.labels is None) or (a.truth is not None and not (len(a.truth) == len(a.labels) == len(a.videos))):
        raise SystemExit("tools/detect.py: --truth and --labels go together, one of each per video file")
    if a.truth_boxes is not None:
        if a.truth is not None:
            raise SystemExit("tools/detect.py: --truth and --truth_boxes exclude each other")
        if a.labels is None or not (len(a.truth_boxes) == len(a.labels) == len(a.videos)):
            raise SystemExit("tools/detect.py: --truth_boxes and --labels go together, one of each per video file")
    if a.actors is not None and (a.truth_boxes is None or not 1 <= a.actors <= 32):
        raise SystemExit("tools/detect.py: --actors A (1..32) numbers the slots of --truth_boxes")
    if a.boxes and not a.score:
        raise SystemExit("tools/detect.py: --boxes is the truth of --score as boxes")
    if a.score and a.videos:
        raise SystemExit("tools/detect.py: --score is for the synthetic videos; give --truth and --labels for video files")
    if a.sweep is not None:
        if a.truth is None and a.truth_boxes is None and not a.score:
            raise SystemExit("tools/detect.py: --sweep scores against truth: give --truth (or --truth_boxes) and --labels, or --score with synthetic videos")
        try:
            detect.threshold_words(a.sweep or None)
        except ValueError as e:
            raise SystemExit("tools/detect.py: --sweep: %s" % e)
    if a.recut and a.sweep is None:
        raise SystemExit("tools/detect.py: --recut cuts at the best threshold of a sweep: give --sweep")
    if a.threshold is not None:
        try:
            detect.cut_word(a.threshold)
        except ValueError as e:
            raise SystemExit("tools/detect.py: --threshold: %s" % e)
    if a.instance_scores and a.instances <= 0:
        raise SystemExit("tools/detect.py: --instance_scores needs --instances K with K > 0 (the scores are reduced per instance)")
    if a.instance_links and a.instances <= 0:
        raise SystemExit("tools/detect.py: --instance_links needs --instances K with K > 0 (the overlaps are counted between instances)")
    if a.link == "mask" and a.instance_links <= 0:
        raise SystemExit("tools/detect.py: --link mask needs --instance_links L with L > 0 (the mask IoU comes from the overlaps)")
    if a.link == "mask" and a.max_gap > a.instance_links - 1:
        raise SystemExit("tools/detect.py: --link mask with --max-gap %d needs --instance_links %d or more" % (a.max_gap, a.max_gap + 1))
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect.py needs a GPU: the hot path is HIP-only (no CPU fallback)")
    if a.ckpt:
        state = torch.load(a.ckpt, map_location="cpu")
        state = state.get("state_dict", state) if isinstance(state, dict) and "format" not in state else state
        try:
            state = trainstate.model_state_of(state)        # a bare state_dict, or the model part of a training-state file
        except ValueError as e:
            raise SystemExit("tools/detect.py: --ckpt %s: %s" % (a.ckpt, e))
        state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
    else:
        state = synthetic.init_state(47, a.classes)
    names = list(a.videos)
    if names:
        videos = [np.load(n) for n in names]
        truths, labels = ([np.load(t) for t in a.truth], list(a.labels)) if a.truth else (None, None)
        if a.truth_boxes:
            try:
                truths, labels = [], list(a.labels)
                for v, t in zip(videos, a.truth_boxes):
                    b = np.load(t)
                    truths.append(evalstep.BoxTruth.from_xywh(b, v.shape[1], v.shape[2], None if a.actors is None else np.arange(1, b.shape[1] + 1)))
            except (ValueError, IndexError) as e:
                raise SystemExit("tools/detect.py: --truth_boxes %s: %s" % (t, e))
    else:
        n = a.synthetic or 4
        made = (synthetic.make_eval_videos_boxes if a.boxes else synthetic.make_eval_videos_u8)(n, num_classes=a.classes, hw=a.hw)
        videos = [v[0] for v in made]
        truths, labels = ([v[1] for v in made], [v[2] for v in made]) if a.score else (None, None)
        names = ["synthetic_%d" % i for i in range(n)]
    engine = detect.DetectEngine(bs=a.bs, hw=a.hw, num_classes=a.classes, state=state, pack=a.pack, masks=a.masks or a.mask_runs or a.instances > 0 or truths is not None, tile=a.tile,
                                 flip=a.flip, instances=a.instances, min_area=a.min_area, conn=a.conn, instance_maps=a.instance_maps,
                                 instance_scores=a.instance_scores, instance_links=a.instance_links)
    if a.frame_size:
        try:
            engine.set_working_frame(tuple(a.frame_size), a.interp)
        except ValueError as e:
            raise SystemExit("tools/detect.py: --frame_size: %s" % e)
    if a.hop is not None:
        try:
            engine.set_clip_hop(a.hop)
        except ValueError as e:
            raise SystemExit("tools/detect.py: --hop: %s" % e)
    if a.sweep is not None:
        engine.set_keep_probs(True)
    if a.threshold is not None:
        engine.set_mask_threshold(a.threshold)
    engine.begin()
    for v in videos:
        engine.add_video(v)
    out = {"names": np.array(names), "tile": np.bool_(a.tile), "flip": np.bool_(a.flip)}
    dets = engine.results()

    def sweep():
        """Print and store the sweep -> the best threshold, None when every f-mAP@0.5 is NaN."""
        sw = engine.sweep(truths, labels, a.sweep or None)
        with np.errstate(invalid="ignore", divide="ignore"):          # printed as below: the mean over the classes that hold a video
            fm = np.array([np.nanmean(r["frame_ious"] / r["n_tot_frames"], axis=0)[10] for r in sw.results])
            vm = np.array([np.nanmean(r["video_ious"] / r["n_vids"], axis=0)[10] for r in sw.results])
            tp, fp, fn = (sw.pixel[:, j].astype(np.float64) for j in range(3))
            prec, rec = tp / (tp + fp), tp / (tp + fn)                # NaN where nothing is predicted / nothing is true
        best = -1 if np.isnan(fm).all() else int(np.nanargmax(fm))
        print("sweep of the mask threshold (%d videos, %d without truth):  threshold  f-mAP@0.5  v-mAP@0.5  pixel precision  pixel recall" % (len(sw.videos), sw.n_skipped))
        for k, t in enumerate(sw.thresholds):
            print("  %s %.4f  %.4f  %.4f  %.4f  %.4f" % ("*" if k == best else " ", t, fm[k], vm[k], prec[k], rec[k]))
        out.update({"sweep_thresholds": sw.thresholds, "sweep_words": sw.words, "sweep_fmAP": sw.fmAP, "sweep_vmAP": sw.vmAP, "sweep_pixel": sw.pixel})
        return None if best < 0 else float(sw.thresholds[best])

    if a.recut and truths is not None:                                # the sweep first: what follows is stored at its best threshold
        t = sweep()
        if t is None:
            print("no best threshold (every f-mAP@0.5 is NaN): the pass stays as it was cut")
        else:
            dets = engine.recut(t)
            print("re-cut on the device at the best threshold %.6f (word %d)" % dets[0].threshold)
    if dets and dets[0].threshold is not None:
        out.update({"mask_threshold": np.float64(dets[0].threshold[0]), "mask_word": np.int32(dets[0].threshold[1])})
    if a.mask_runs:
        for key, which in (("mask", "masks"),) + ((("imap", "imap"),) if a.instances and a.instance_maps else ()):
            for i, r in enumerate(engine.mask_runs(which)):
                out.update({"%s_runs_%d" % (key, i): r.runs, "%s_run_offsets_%d" % (key, i): r.offsets, "%s_shape_%d" % (key, i): np.array(r.shape, np.int64)})
    if truths is not None:
        ps = engine.score(truths, labels, actors=a.actors or 1)
        r = ps.result
        with np.errstate(invalid="ignore", divide="ignore"):          # printed: the mean over the classes that hold a video (the stored fmAP / vmAP are
            fm = np.nanmean(r["frame_ious"] / r["n_tot_frames"], axis=0)  # the evaluator's, NaN as soon as one class holds none)
            vm = np.nanmean(r["video_ious"] / r["n_vids"], axis=0)
        print("score against truth (classes with a video): f-mAP@0.2 %.4f  f-mAP@0.5 %.4f  v-mAP@0.2 %.4f  v-mAP@0.5 %.4f  accuracy %.4f  (%d videos, %d without truth)"
              % (fm[4], fm[10], vm[4], vm[10], r["accuracy"], len(ps.videos), ps.n_skipped))
        out.update({"score_" + k: np.asarray(v) for k, v in r.items()})
        for i, v in enumerate(ps.videos):
            out.update({"score_table_%d" % i: v.table, "score_counts_%d" % i: v.counts, "score_label_%d" % i: np.int32(v.label)})
    if a.sweep is not None and truths is not None and not a.recut:
        sweep()
    for i, (name, d) in enumerate(zip(names, dets)):
        tubes = d.tubes(a.min_pixels, a.max_gap)
        out.update({"label_%d" % i: np.int32(d.label), "class_scores_%d" % i: d.class_scores, "counts_%d" % i: d.counts, "boxes_%d" % i: d.boxes,
                    "frame_scores_%d" % i: d.frame_scores, "views_%d" % i: np.array(d.views, np.int32).reshape(-1, 3),
                    "tubes_%d" % i: np.array([(t0, t1, s) for t0, t1, _b, s in tubes], np.float64).reshape(-1, 3)})
        if d.work is not None:
            out["work_%d" % i] = np.array([d.work[0], d.work[1], detect.INTERPOLATIONS[d.work[2]]], np.int32)
        if d.hop is not None:
            out["hop_%d" % i] = np.int32(d.hop)
        if a.masks:
            m = d.masks.cpu().numpy()
            out.update({"masks_%d" % i: np.packbits(m), "mask_shape_%d" % i: np.array(m.shape, np.int64)})
        itubes = []
        if a.instances:
            itubes = d.instance_tubes(max_gap=a.max_gap, link=a.link)
            out.update({"inst_n_%d" % i: d.inst_n, "inst_kept_%d" % i: d.inst_kept, "inst_flags_%d" % i: d.inst_flags, "inst_areas_%d" % i: d.inst_areas,
                        "inst_boxes_%d" % i: d.inst_boxes, "inst_first_%d" % i: d.inst_first,
                        "inst_tubes_%d" % i: np.array([(t0, t1, s) for t0, t1, _b, _a, s in itubes], np.float64).reshape(-1, 3),
                        "inst_tube_boxes_%d" % i: np.concatenate([t[2] for t in itubes] + [np.zeros((0, 4), np.int32)]).astype(np.int32)})
            if d.inst_scores is not None:
                out.update({"inst_scores_%d" % i: d.inst_scores, "other_score_%d" % i: d.other_score})
            if d.inst_overlaps is not None:
                out["inst_overlaps_%d" % i] = d.inst_overlaps
            if d.imap is not None and not a.mask_runs:
                m = d.imap.cpu().numpy()
                out.update({"imap_%d" % i: m, "imap_shape_%d" % i: np.array(m.shape, np.int64)})
        print("%s: %d frames, class %d (%.4f), %d frames detected, %d tube(s)%s%s" % (
            name, d.counts.size, d.label, d.class_score, int((d.counts >= a.min_pixels).sum()), len(tubes),
            "".join("  [%d..%d] %.3f" % (t0, t1, s) for t0, t1, _b, s in tubes[:4]),
            "; %d instances in %d instance tube(s), %d frame(s) over the run cap" % (int(d.inst_kept.sum()), len(itubes), int((d.inst_flags & 1).sum()))
            if a.instances else ""))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d videos, %d clips)" % (a.out, len(names), engine.n_clips))


if __name__ == "__main__":
    main()
