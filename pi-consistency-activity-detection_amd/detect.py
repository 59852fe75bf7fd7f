"""Detection output on one MI355X: where the action is in a video and which action it is, from DECODED uint8 video without truth.  The
inference side of evalstep.EvalEngine -- the same upload pool, clip kernel (pc_clips_from_u8_views: the truth side compiled out), single eval plan
whose weight layouts are made once per pass, and class-score ring -- ending not in hit tables but in detections: behind each batch one
pc_detect_frames per video segment undoes the clip interleave (frame k of a clip is start + k * f_skip) straight into the video's uint8 masks
in frame order and full-frame coordinates and leaves one record per frame (pixel count, box, score); behind a video's last clip
pc_video_class votes its class, and one asynchronous copy takes records and class vector into page-locked memory.  No truth, no flag
kernel, and the compute stream is never waited for per video (the host only waits for the upload of two videos ago to have left its
page-locked slot): `results()` is the one host wait of a pass.  The masks stay on the device.

The mask predicate is the evaluator's own (fp32 sigmoid(x) >= 0.5, one device function for both kernels), so a detection and the f-mAP /
v-mAP that scores it cannot disagree on a pixel.  The model localises one actor per clip, as the reference's does: a tube is a run of
detected frames, its class and class score are the video's.

Views.  By default the network sees the centre hw x hw crop of every frame, as the reference's evaluator does.  With tile / flip / views a
video is cut into several VIEWS (h0, w0, flip) -- crops at their own offsets, optionally mirrored left-right; the model is trained on random
crops and its consistency loss ties the map of a clip to the map of its mirror image -- every view runs through the same plan, and
pc_detect_frames_views merges their logits per full-frame pixel (the mean over the views that cover the pixel) in front of the threshold,
the box and the score: one pc_clips_from_u8_views launch in front of the forward and one merge launch behind it per video segment.

Instances.  One box per frame is stretched across the image by a single false-positive pixel and holds every actor of a multi-actor video.
With instances=K one pc_frame_instances launch per video, behind its last clip, splits every frame's mask into its connected components on the
device and leaves the K largest per frame (area, box, first pixel) next to the records; link_instance_tubes links them across frames into
per-actor tubes by box IoU.

Instance scores.  With instance_scores=True one pc_frame_probs launch behind each pc_detect_frames* keeps the per-pixel probability of the
merged logit (uint16, video order; the merge is one device function for mask and probability) until the video's last clip, where one
pc_instance_scores launch behind pc_frame_instances reduces it per instance: every instance, and with it every per-actor tube, carries the mean
probability of its own pixels instead of the frame's.

Instance links.  Box IoU swaps two actors whose boxes overlap as soon as their area ranks change.  With instance_links=L one
pc_instance_overlaps launch behind pc_frame_instances counts, for every frame and each of the L frame distances, the pixels every instance
shares with every instance of the later frame; link_instance_tubes_by_mask links by the mask IoU that follows from them.

Mask runs.  The masks (and the maps of ranks) stay on the device; DetectEngine.mask_runs, called after results(), brings those of a whole
pass to the host as row runs -- pc_mask_run_index / pc_mask_runs per video, two host waits per call -- in MaskRuns objects: a frame of a
few blobs is 1-2 KB instead of its H * W bytes.

Score.  DetectEngine.score(truths, labels), called after results(), measures a pass against truth masks: one pc_map_crosstab launch per video
cross-tabulates its mask (or map of ranks) with the truth on the device, all tables leave in one copy -- one host wait per call -- and the
host turns them into the evaluator's own f-mAP / v-mAP tables (crosstab_counts, accumulate_video) and a per-instance IoU against truth
actors (instance_actor_iou), in VideoScore / PassScore objects.  Unlike evalstep.EvalEngine, whose protocol is the centre crop, the truth is
taken on the FULL frame, so a tiled or mirrored pass can be scored; and the class vote is the detection's, over all clips of the video,
where EvalEngine votes over the clips that hold truth.

Working frame.  The crops are cut at the video's own pixel scale unless DetectEngine.set_working_frame((Hs, Ws), interpolation) is called: then
every video is resized on the device to Hs x Ws (pc_resize_u8: cv2.resize restated), the views are crops of that working frame, and
pc_detect_frames_scaled merges them there and resamples the merged logits bilinearly to every native pixel in front of the threshold, the
box, the score and the probability -- masks, records, instances, runs and score() stand in native coordinates at native size as before.

Sweep.  The mask is cut at sigmoid(x) >= 0.5; whether that is the right operating point is what DetectEngine.sweep(truths, labels,
thresholds), called after results(), answers from the probability maps of a pass (set_keep_probs, or instance_scores=True): one
pc_prob_truth_hist launch per video counts its pixels by (truth or not, how many of the N threshold words lie at or below the probability
word), all histograms leave in one copy -- one host wait per call -- and the host turns their suffix sums into the (inter, union, gt) of every
threshold (sweep_counts) and those into f-mAP / v-mAP per threshold through the evaluator's own accumulate_video, in a SweepScore.

Clip hop.  A video is cut into windows of 8 * f_skip frames that start every 8 * f_skip frames, so every frame is decided by one forward,
unless DetectEngine.set_clip_hop(hop) is called: then the windows start every `hop` frames (clip_starts_hop), a frame lies in up to
ceil(8 * f_skip / hop) of them, pc_clip_planes keeps the merged logits of every (window, frame) on the device until the video's last clip has
run, and pc_detect_frames_planes averages the windows that hold a frame in front of the resample, the threshold, the box, the score and the
probability.  Everything behind mask, probability and record -- instances, scores, links, runs, score() -- works on them unchanged.

Mask threshold.  What sweep() finds the engine can use: DetectEngine.set_mask_threshold(t) has the videos to come cut at the word
cut_word(t) -- the sweep's own word for t -- by one pc_prob_cut launch per video over its kept probability map, behind its last clip and in
front of the class vote and the instances: the mask is q >= word (pc_prob_truth_hist's "positive at threshold k"), count, box and score of
the records are made from it, and everything behind a mask runs on it unchanged.  DetectEngine.recut(t), called after results(), cuts the
pass that just ran again at t on the device, with no second forward and one host wait: recut(sw.thresholds[k]) followed by score() gives
sw.results[k] bit for bit.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import evalmetrics, ops
from .evalstep import BoxTruth, ClipEngine, _as_u8, centre_crop, check_counts, check_label, check_truth, clip_starts, ring_place

PIN_CHUNK_WORDS = 1 << 18          # page-locked staging of the records, 1 MiB at a time
MAX_VIEWS = ops.MAX_VIEWS          # views of one video (one launch cuts, one merges, all of them)
INTERPOLATIONS = {"nearest": 0, "linear": 1, "area": 3}      # set_working_frame: the cv2 flags ops.resize_u8 takes


# ---------------------------------------------------------------------- pure host functions (tests/test_detect_cpu.py)
def link_tubes(counts, boxes, frame_scores, min_pixels=1, max_gap=0):
    """Per-frame records -> action tubes.  A tube is a maximal run of frames with count >= min_pixels; two runs merge when at most max_gap
    frames lie between them (those frames keep their box as it is: empty, for a frame without a positive pixel).
    -> [(t0, t1, boxes[t0:t1 + 1], score)], t1 inclusive, score the float64 mean of the frame scores of the tube's DETECTED frames."""
    counts = np.asarray(counts).reshape(-1)
    boxes = np.asarray(boxes).reshape(-1, 4)
    scores = np.asarray(frame_scores, np.float64).reshape(-1)
    if not (counts.size == boxes.shape[0] == scores.size):
        raise ValueError("link_tubes: %d counts, %d boxes, %d scores" % (counts.size, boxes.shape[0], scores.size))
    if min_pixels < 1 or max_gap < 0:
        raise ValueError("link_tubes: min_pixels >= 1 and max_gap >= 0, got %r and %r" % (min_pixels, max_gap))
    on = counts >= min_pixels
    runs = []
    for t in np.flatnonzero(on).tolist():
        if runs and t - runs[-1][1] - 1 <= max_gap:
            runs[-1][1] = t
        else:
            runs.append([t, t])
    return [(t0, t1, boxes[t0:t1 + 1].copy(), float(scores[t0:t1 + 1][on[t0:t1 + 1]].mean())) for t0, t1 in runs]


def box_iou(a, b):
    """IoU of two half-open boxes x0, y0, x1, y1 (float; 0.0 when either is empty)."""
    iw, ih = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    if iw <= 0 or ih <= 0:
        return 0.0
    inter = float(iw) * float(ih)
    return inter / (float(a[2] - a[0]) * float(a[3] - a[1]) + float(b[2] - b[0]) * float(b[3] - b[1]) - inter)


def link_instance_tubes(inst_kept, inst_boxes, inst_areas, frame_scores, iou_min=0.3, max_gap=0, min_len=1, inst_scores=None):
    """Per-frame instances -> per-actor tubes, greedily and deterministically.  inst_kept [F], inst_boxes [F,K,4], inst_areas [F,K] as
    Detection holds them (rank order), frame_scores [F].  Frames are taken in order and the open tubes in the order they were opened: each
    tube takes the not-yet-taken instance of the frame with the highest box IoU against its last box, if that IoU >= iou_min (a tie goes to
    the lower rank); instances no tube took open new tubes in rank order.  A tube closes once it has gone unmatched for more than max_gap
    frames; a bridged frame carries an empty box and area 0.  Tubes with fewer than min_len detected frames are dropped.
    -> [(t0, t1, boxes[t1 - t0 + 1, 4], areas[t1 - t0 + 1], score)] in the order the tubes were opened, t1 inclusive (the last DETECTED frame),
    score the float64 mean of frame_scores over the tube's detected frames -- or, with inst_scores [F,K] (Detection.inst_scores), the float64
    mean of the scores of the tube's own instances over those frames; the linking is the same either way.  iou_min = 0.3 is an API default,
    not a measured quantity."""
    return _link_instances("link_instance_tubes", inst_kept, inst_boxes, inst_areas, frame_scores, iou_min, max_gap, min_len, inst_scores,
                           lambda boxes, areas: lambda tb, t, r: box_iou(tb["box"], boxes[t, r]))


def link_instance_tubes_by_mask(inst_kept, inst_boxes, inst_areas, frame_scores, overlaps, inst_flags=None, iou_min=0.3, max_gap=0, min_len=1,
                                inst_scores=None):
    """link_instance_tubes with the MASK IoU as its measure: the same greedy, deterministic procedure, order, max_gap / min_len / score rules
    and return tuples; only what is compared differs.  overlaps int32 [F, L, K + 1, K + 1] (Detection.inst_overlaps: overlaps[f, l, a, b] the
    pixels slot a of frame f shares with slot b of frame f + l + 1).  Between a tube's last detected instance (frame tl, rank ra) and the
    candidate (t, rb): inter = overlaps[tl, t - tl - 1, slot(tl, ra), slot(t, rb)], IoU = inter / (area_a + area_b - inter) in float64, 0
    when that denominator is 0.  slot(f, r) = r, except in a frame whose inst_flags bit 0 is set (overflow: its map is 255 on all
    foreground and its one substituted instance holds the frame's count): there it is K.  Slot K of any other frame is foreground no
    instance holds and links nothing.  max_gap > L - 1: ValueError, no record exists for that lag."""
    who = "link_instance_tubes_by_mask"
    ov = np.asarray(overlaps)
    kept = np.asarray(inst_kept).reshape(-1)
    F = kept.size
    if F == 0:
        return []
    K = np.asarray(inst_boxes).reshape(F, -1, 4).shape[1]
    if ov.ndim != 4 or ov.shape[0] != F or ov.shape[1] < 1 or ov.shape[2:] != (K + 1, K + 1):
        raise ValueError("%s: overlaps %s, expected [%d, L, %d, %d]" % (who, ov.shape, F, K + 1, K + 1))
    if max_gap > ov.shape[1] - 1:
        raise ValueError("%s: max_gap = %r needs the overlaps of %d lags, the record holds %d" % (who, max_gap, max_gap + 1, ov.shape[1]))
    over = np.zeros(F, bool)
    if inst_flags is not None:
        flags = np.asarray(inst_flags).reshape(-1)
        if flags.size != F:
            raise ValueError("%s: %d flags for %d frames" % (who, flags.size, F))
        over = (flags & 1) != 0

    def measure(boxes, areas):
        def mask_iou(tb, t, r):
            tl, ra = tb["last"], tb["rank"]
            inter = int(ov[tl, t - tl - 1, K if over[tl] else ra, K if over[t] else r])
            union = int(areas[tl, ra]) + int(areas[t, r]) - inter
            return float(inter) / float(union) if union != 0 else 0.0
        return mask_iou
    return _link_instances(who, inst_kept, inst_boxes, inst_areas, frame_scores, iou_min, max_gap, min_len, inst_scores, measure)


def _link_instances(who, inst_kept, inst_boxes, inst_areas, frame_scores, iou_min, max_gap, min_len, inst_scores, make_measure):
    """The loop of link_instance_tubes and link_instance_tubes_by_mask.  make_measure(boxes, areas) -> measure(tube, t, r): how well the
    instance of rank r in frame t continues the tube (a dict with its last detected frame `last`, that instance's `rank` and `box`)."""
    kept = np.asarray(inst_kept).reshape(-1)
    F = kept.size
    if F == 0:
        return []
    boxes = np.asarray(inst_boxes).reshape(F, -1, 4)
    areas = np.asarray(inst_areas).reshape(F, -1)
    scores = np.asarray(frame_scores, np.float64).reshape(-1)
    if not (areas.shape[1] == boxes.shape[1] and scores.size == F) or kept.max() > boxes.shape[1]:
        raise ValueError("%s: %d frames, boxes %s, areas %s, %d scores" % (who, F, boxes.shape, areas.shape, scores.size))
    if inst_scores is not None:
        inst_scores = np.asarray(inst_scores, np.float64).reshape(F, -1)
        if inst_scores.shape[1] != boxes.shape[1]:
            raise ValueError("%s: inst_scores %s against boxes %s" % (who, inst_scores.shape, boxes.shape))
    if not 0.0 <= iou_min <= 1.0 or max_gap < 0 or min_len < 1:
        raise ValueError("%s: 0 <= iou_min <= 1, max_gap >= 0, min_len >= 1, got %r, %r, %r" % (who, iou_min, max_gap, min_len))
    measure = make_measure(boxes, areas)
    tubes, live = [], []                                  # a tube: dict(t0, frames {t: rank}, last box, last rank, last t)
    for t in range(F):
        n = int(kept[t])
        taken = [False] * n
        still = []
        for tb in live:
            best, best_iou = -1, -1.0
            for r in range(n):
                if not taken[r]:
                    v = measure(tb, t, r)
                    if v >= iou_min and v > best_iou:
                        best, best_iou = r, v
            if best >= 0:
                taken[best] = True
                tb["frames"][t] = best
                tb["box"], tb["rank"], tb["last"] = boxes[t, best], best, t
            if t - tb["last"] <= max_gap:
                still.append(tb)
        live = still
        for r in range(n):
            if not taken[r]:
                tb = dict(t0=t, frames={t: r}, box=boxes[t, r], rank=r, last=t)
                tubes.append(tb)
                live.append(tb)
    out = []
    for tb in tubes:
        if len(tb["frames"]) < min_len:
            continue
        t0, t1 = tb["t0"], tb["last"]
        bx, ar = np.zeros((t1 - t0 + 1, 4), boxes.dtype), np.zeros(t1 - t0 + 1, areas.dtype)
        for t, r in tb["frames"].items():
            bx[t - t0], ar[t - t0] = boxes[t, r], areas[t, r]
        det = sorted(tb["frames"])
        score = scores[det].mean() if inst_scores is None else inst_scores[det, [tb["frames"][t] for t in det]].mean()
        out.append((t0, t1, bx, ar, float(score)))
    return out


def clip_starts_hop(F, f_skip, hop):
    """The clip starts of a video of F frames cut into overlapping windows (csrc/cliphop.h, restated; tests/test_clip_hop_cpu.py holds the
    two to each other): windows of span = 8 * f_skip frames start every `hop` frames, hop a multiple of f_skip in [f_skip, span]; window i
    is kept iff i == 0 or i - hop + span < F (stop behind the first window that reaches the video's end); the starts are i + j for every
    kept window and phase j < f_skip with i + j < F, in that order.  hop == span: evalstep.clip_starts(F, ones, f_skip)."""
    span = 8 * f_skip
    if F < 1 or not 1 <= f_skip <= 1 << 20 or hop % f_skip or not f_skip <= hop <= span:      # (2^20: the library's bound on f_skip)
        raise ValueError("clip_starts_hop: F = %r, f_skip = %r, hop = %r (F >= 1, hop a multiple of f_skip in [f_skip, 8 * f_skip])" % (F, f_skip, hop))
    return [i + j for i in range(0, F, hop) if i == 0 or i - hop + span < F for j in range(f_skip) if i + j < F]


def _tile_offsets(L, hw):
    nt = -(-L // hw)
    return [0] if nt == 1 else [(i * (L - hw)) // (nt - 1) for i in range(nt)]


def check_views(views, H, W, hw):
    """Views given by a caller -> [(h0, w0, flip)] as ints, or ValueError: 1..MAX_VIEWS of them, every crop inside the frame, flip 0 or 1."""
    try:
        out = [(int(h0), int(w0), int(fl)) for h0, w0, fl in views]
    except (TypeError, ValueError):
        raise ValueError("views: a list of (h0, w0, flip), got %r" % (views,)) from None
    if not 1 <= len(out) <= MAX_VIEWS:
        raise ValueError("%d views for frames of %d x %d: 1..%d are allowed" % (len(out), H, W, MAX_VIEWS))
    for h0, w0, fl in out:
        if h0 < 0 or w0 < 0 or h0 + hw > H or w0 + hw > W or fl not in (0, 1):
            raise ValueError("view (%d, %d, %d): a %d x %d crop outside the %d x %d frame, or flip not 0 / 1" % (h0, w0, fl, hw, hw, H, W))
    return out


def make_views(H, W, hw, tile=False, flip=False):
    """The views (h0, w0, flip) of an H x W frame for a network of hw x hw.  tile=False: the centre crop.  tile=True: each axis of length L
    gets ceil(L / hw) crops at the offsets (i * (L - hw)) // (nt - 1), so that every frame pixel is covered; y-major, x-minor.  flip=True: each
    crop is followed directly by its mirrored twin.  More than MAX_VIEWS views: ValueError."""
    if hw < 1 or H < hw or W < hw:
        raise ValueError("frames of %d x %d are smaller than the %d x %d crop" % (H, W, hw, hw))
    tiles = [(h0, w0) for h0 in _tile_offsets(H, hw) for w0 in _tile_offsets(W, hw)] if tile else [centre_crop(H, W, hw)]
    views = [(h0, w0, fl) for h0, w0 in tiles for fl in ((0, 1) if flip else (0,))]
    if len(views) > MAX_VIEWS:
        raise ValueError("frames of %d x %d at hw = %d need %d views, more than the %d allowed" % (H, W, hw, len(views), MAX_VIEWS))
    return views


class Detection:
    """One video's detections.  label / class_score / class_scores [C]: the arg-max of the mean class scores of its clips, that mean, all means;
    counts [F] positive pixels, boxes [F, 4] = x0, y0, x1, y1 (half-open, full-frame coordinates, zeros for an empty frame) and frame_scores [F]
    (mean sigmoid over the positive pixels) per frame; masks: device uint8 [F, H, W] or None; views: the (h0, w0, flip) the video was seen
    through; work: None, or (Hs, Ws, interpolation) when the video was resized to a working frame (DetectEngine.set_working_frame) -- the
    views are then in WORKING-frame coordinates, everything else in native ones; hop: None, or the distance between two windows when the
    video was cut into overlapping clips (DetectEngine.set_clip_hop) -- class_scores are then the mean over the rows of ALL its clips.

    With DetectEngine(instances=K) also the frame's connected components of at least min_area pixels, ranked by area (ties: the first pixel in
    raster order): inst_n [F] how many there are, inst_kept [F] = min(inst_n, K) how many are held, inst_flags [F] (bit 0: the frame had more
    row runs than the kernel labels -- it then holds ONE instance, the frame's own count and box, with first = -1), inst_areas [F, K],
    inst_boxes [F, K, 4], inst_first [F, K] (y * W + x of the component's first pixel; zeros from inst_kept on), and imap: device uint8
    [F, H, W] with 0 background, r + 1 on the instance of rank r, 255 on other foreground (instance_maps=True), else None.  All None without
    instances.

    With DetectEngine(instance_scores=True) also inst_scores float64 [F, K], the mean probability over the instance's own pixels (zeros from
    inst_kept on; the one instance of an overflow frame: over all of the frame's foreground), other_score float64 [F], that mean over the
    foreground no kept instance holds (0 when there is none), and probs: the device 16-bit [F, H, W] probability map, uint16 steps of
    1 / 65535.  All None without the option.

    With DetectEngine(instance_links=L) also inst_overlaps int32 [F, L, K + 1, K + 1]: inst_overlaps[f, l, a, b] the pixels that slot a of
    frame f shares with slot b of frame f + l + 1 (slot r < K: the instance of rank r; slot K: all other foreground, and ALL foreground of a
    frame whose overflow flag is set; zeros where frame f + l + 1 does not exist).  None without the option.

    threshold: None for a video whose mask is seg_positive's (fp32 sigmoid(x) >= 0.5), or (threshold, word) when it was cut from its
    probability map at q >= word (DetectEngine.set_mask_threshold / recut).  The frame_scores of a cut video are means of the probability
    WORDS of the positive pixels / 65535, not of the fp32 sigmoid: a word is the sigmoid rounded to a step of 1 / 65535, so the two differ
    by at most half a step plus the rounding of the float32 result, below 1e-5 -- the bound instance scores carry."""

    work = None                          # set by DetectEngine.results() behind the constructor, whose parameter list is pinned
    hop = None                           # likewise
    threshold = None                     # likewise (and by DetectEngine.recut)

    def __init__(self, label, class_score, class_scores, counts, boxes, frame_scores, masks, views=None, inst=None, imap=None, scores=None, probs=None,
                 inst_overlaps=None):
        self.label, self.class_score, self.class_scores = label, class_score, class_scores
        self.counts, self.boxes, self.frame_scores, self.masks, self.views = counts, boxes, frame_scores, masks, views
        self.inst_n, self.inst_kept, self.inst_flags, self.inst_areas, self.inst_boxes, self.inst_first = inst if inst is not None else (None,) * 6
        self.imap = imap
        self.inst_scores, self.other_score = scores if scores is not None else (None, None)
        self.probs = probs
        if inst_overlaps is not None:
            inst_overlaps = np.asarray(inst_overlaps)
            K = None if self.inst_areas is None else int(np.asarray(self.inst_areas).shape[-1])
            if K is None or inst_overlaps.ndim != 4 or inst_overlaps.shape[0] != len(self.counts) or inst_overlaps.shape[2:] != (K + 1, K + 1):
                raise ValueError("Detection: inst_overlaps %s need instances and the shape [F, L, K + 1, K + 1]" % (inst_overlaps.shape,))
        self.inst_overlaps = inst_overlaps

    def tubes(self, min_pixels=1, max_gap=0):
        return link_tubes(self.counts, self.boxes, self.frame_scores, min_pixels, max_gap)

    def instance_tubes(self, iou_min=0.3, max_gap=0, min_len=1, link="box"):
        """The per-actor tubes: link="box" by box IoU (link_instance_tubes), link="mask" by mask IoU from inst_overlaps
        (link_instance_tubes_by_mask; max_gap at most L - 1)."""
        if link not in ("box", "mask"):
            raise ValueError("instance_tubes: link = %r, \"box\" or \"mask\"" % (link,))
        if self.inst_kept is None:
            raise ValueError("instance_tubes: the detection holds no instances (DetectEngine(instances=K))")
        if link == "mask":
            if self.inst_overlaps is None:
                raise ValueError("instance_tubes: link=\"mask\" needs the overlaps of DetectEngine(instance_links=L); the detection holds none")
            return link_instance_tubes_by_mask(self.inst_kept, self.inst_boxes, self.inst_areas, self.frame_scores, self.inst_overlaps, self.inst_flags,
                                               iou_min, max_gap, min_len, self.inst_scores)
        return link_instance_tubes(self.inst_kept, self.inst_boxes, self.inst_areas, self.frame_scores, iou_min, max_gap, min_len, self.inst_scores)


RUN_RANGE_ROWS, RUN_RANGE_PIXELS = ops.RUN_MAX_ROWS, ops.RUN_MAX_PIXELS      # what one pc_mask_run_index / pc_mask_runs range may hold


class MaskRuns:
    """One video's mask (or map of ranks) as row runs, on the host.  shape = (F, H, W); runs uint32 [n, 2] in raster order over the whole
    video: runs[i] = (row | value << 24, x0 | x1 << 16) with row = f * H + y, the columns x0 .. x1 - 1 and the pixels' byte value (1 for a
    mask; rank + 1 or 255 for a map of ranks) -- the words pc_mask_runs writes; offsets int64 [F + 1]: frame f holds the runs
    offsets[f] .. offsets[f + 1] - 1.  A run is a maximal horizontal segment of one non-zero value: value 0 belongs to no run."""

    def __init__(self, shape, offsets, runs):
        F, H, W = (int(v) for v in shape)
        self.shape = (F, H, W)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        runs = np.ascontiguousarray(runs)
        if runs.dtype not in (np.uint32, np.int32):
            raise ValueError("MaskRuns: runs must be 32-bit words, got %s" % runs.dtype)
        self.runs = runs.view(np.uint32).reshape(-1, ops.RUN_WORDS)
        if F < 1 or H < 1 or not 1 <= W <= 65535 or F * H > ops.RUN_MAX_ROWS:
            raise ValueError("MaskRuns: %d frames of %d x %d: W <= 65535 and F * H <= 2^24 (the row field of a run)" % (F, H, W))
        if self.offsets.size != F + 1 or self.offsets[0] != 0 or self.offsets[-1] != self.runs.shape[0] or (np.diff(self.offsets) < 0).any():
            raise ValueError("MaskRuns: offsets %s do not split %d runs over %d frames" % (self.offsets.shape, self.runs.shape[0], F))

    @classmethod
    def from_dense(cls, array):
        """The runs of a uint8 array [F, H, W] (or one frame [H, W]), encoded on the host: the format the device writes."""
        a = np.asarray(array)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError("MaskRuns.from_dense: uint8 [F, H, W] or [H, W], got %s %s" % (a.dtype, a.shape))
        a = a.reshape((-1,) + a.shape[-2:])
        F, H, W = a.shape
        rows = np.zeros((F * H, W + 2), np.int16)                     # a zero in front of and behind every row
        rows[:, 1:-1] = a.reshape(F * H, W)
        change = rows[:, 1:] != rows[:, :-1]                          # change[r, x]: pixel x differs from pixel x - 1 (x = W: the zero behind)
        sr, sx = np.nonzero(change[:, :-1] & (rows[:, 1:-1] != 0))    # starts: non-zero and unlike the pixel to the left
        er, ex = np.nonzero(change[:, 1:] & (rows[:, 1:-1] != 0))     # ends: non-zero and unlike the pixel to the right; the j-th end closes the j-th start
        runs = np.empty((sr.size, ops.RUN_WORDS), np.uint32)
        runs[:, 0] = sr.astype(np.uint32) | (rows[sr, sx + 1].astype(np.uint32) << 24)
        runs[:, 1] = sx.astype(np.uint32) | ((ex + 1).astype(np.uint32) << 16)
        offsets = np.searchsorted(sr, np.arange(F + 1, dtype=np.int64) * H).astype(np.int64)
        return cls((F, H, W), offsets, runs)

    @property
    def nbytes(self):
        return int(self.runs.nbytes + self.offsets.nbytes)

    def frame(self, f):
        """-> (y, x0, x1, value) int32 arrays of frame f's runs, raster order; x1 half-open."""
        F, H, _W = self.shape
        f = int(f)
        if not 0 <= f < F:
            raise ValueError("MaskRuns.frame: frame %d outside 0..%d" % (f, F - 1))
        r = self.runs[self.offsets[f]:self.offsets[f + 1]]
        return ((r[:, 0] & 0xffffff).astype(np.int32) - f * H, (r[:, 1] & 0xffff).astype(np.int32), (r[:, 1] >> 16).astype(np.int32),
                (r[:, 0] >> 24).astype(np.int32))

    def areas(self):
        """-> int64 [F]: the pixels of every frame's runs, the sum of x1 - x0."""
        length = (self.runs[:, 1] >> 16).astype(np.int64) - (self.runs[:, 1] & 0xffff).astype(np.int64)
        csum = np.concatenate([np.zeros(1, np.int64), np.cumsum(length, dtype=np.int64)])
        return csum[self.offsets[1:]] - csum[self.offsets[:-1]]

    def dense(self, f=None):
        """-> uint8 [H, W] of frame f, or [F, H, W] of the whole video."""
        F, H, W = self.shape
        if f is None:
            return ops.decode_mask_runs(self.runs, F, H, W)
        f = int(f)
        if not 0 <= f < F:
            raise ValueError("MaskRuns.dense: frame %d outside 0..%d" % (f, F - 1))
        r = self.runs[self.offsets[f]:self.offsets[f + 1]].copy()
        r[:, 0] -= np.uint32(f * H)
        return ops.decode_mask_runs(r, 1, H, W)[0]


def run_ranges(F, H, W):
    """The frame ranges (f0, nf) in which a video of F frames of H x W goes through pc_mask_run_index / pc_mask_runs: as few as keep
    nf * H * W below 2^31 and nf * H within 2^24."""
    per = min(RUN_RANGE_PIXELS // (H * W), RUN_RANGE_ROWS // H)
    if per < 1:
        raise ValueError("mask_runs: one frame of %d x %d is beyond what a range holds" % (H, W))
    return [(f0, min(per, F - f0)) for f0 in range(0, F, per)]


# ---------------------------------------------------------------------- a pass against truth (tests/test_detect_score_cpu.py)
def crosstab_counts(table):
    """Tables int32 [F, P + 2, A + 2] of pc_map_crosstab -> int64 [F, 3] = (inter, union, gt) per frame: the pixels that are foreground on both
    sides, on either side, and in the truth -- the triple pc_seg_frame_counts leaves when the truth is in {0, 1}."""
    t = np.asarray(table).astype(np.int64)
    if t.ndim != 3 or t.shape[1] < 2 or t.shape[2] < 2:
        raise ValueError("crosstab_counts: tables [F, P + 2, A + 2], got %s" % (t.shape,))
    out = np.empty((t.shape[0], 3), np.int64)
    out[:, 0] = t[:, 1:, 1:].sum(axis=(1, 2))
    out[:, 1] = t.sum(axis=(1, 2)) - t[:, 0, 0]
    out[:, 2] = t[:, :, 1:].sum(axis=(1, 2))
    return out


def accumulate_video(counts, label, acc):
    """map_accumulate_kernel (csrc/evalmetrics.hip) on the host: one video's counts [F, 3] = (inter, union, gt) into the tables of an
    evalmetrics.MapAccumulator built with device="cpu".  Only frames with gt != 0 count, for the frame tables and for the video's sums; per
    threshold k the float64 ratio inter / union is compared (>=) with the float32 k / 20 widened to float64; video_hits is touched only when
    the summed union is positive; n_vids[label] += 1.  A video without any truth pixel is the caller's to skip (EvalEngine.add_video
    returning 0): it is not passed here."""
    c = np.asarray(counts).astype(np.int64).reshape(-1, 3)
    label = int(label)
    if not 0 <= label < acc.n_classes:
        raise ValueError("accumulate_video: label %d outside [0, %d)" % (label, acc.n_classes))
    fh, vh, nfr, nv = (t.numpy() for t in (acc.frame_hits, acc.video_hits, acc.n_frames, acc.n_vids))      # views: the adds land in the tensors
    on = c[:, 2] != 0
    inter, union = c[on, 0], c[on, 1]
    thr = (np.arange(evalmetrics.N_THR, dtype=np.float32) / np.float32(20.0)).astype(np.float64)
    ratio = inter.astype(np.float64) / union.astype(np.float64)        # union >= gt > 0 on these frames
    fh[label] += (ratio[:, None] >= thr[None, :]).sum(axis=0).astype(np.int32)
    vi, vu = int(inter.sum()), int(union.sum())
    if vu > 0:
        vh[label] += (np.float64(vi) / np.float64(vu) >= thr).astype(np.int32)
    nfr[label] += int(on.sum())
    nv[label] += 1


def instance_actor_iou(table):
    """Tables int32 [F, P + 2, A + 2] -> float64 [F, P, A]: the IoU of the pixels of pred slot r + 1 (the instance of rank r) with those of
    truth slot a + 1 (actor a + 1): inter / (row sum + column sum - inter), 0.0 where that denominator is 0."""
    t = np.asarray(table).astype(np.int64)
    if t.ndim != 3 or t.shape[1] < 3 or t.shape[2] < 3:
        raise ValueError("instance_actor_iou: tables [F, P + 2, A + 2], got %s" % (t.shape,))
    inter = t[:, 1:-1, 1:-1]
    den = t.sum(axis=2)[:, 1:-1, None] + t.sum(axis=1)[:, None, 1:-1] - inter
    return np.where(den != 0, inter.astype(np.float64) / np.maximum(den, 1).astype(np.float64), 0.0)


class VideoScore:
    """One video of a pass against its truth.  table int32 [F, P + 2, A + 2] (pc_map_crosstab); counts int64 [F, 3] = (inter, union, gt);
    frame_iou float64 [F], NaN where the frame holds no truth; video_iou: summed inter / summed union over the frames with truth, NaN for a
    skipped video; label the true class, predicted the detection's, correct whether they agree; skipped: the video holds no truth pixel and
    entered no table (as EvalEngine skips it)."""

    def __init__(self, table, label, predicted):
        self.table = table
        self.counts = crosstab_counts(table)
        self.label, self.predicted = int(label), int(predicted)
        on = self.counts[:, 2] != 0
        self.skipped = not bool(on.any())
        self.correct = not self.skipped and self.label == self.predicted
        self.frame_iou = np.full(self.counts.shape[0], np.nan, np.float64)
        self.frame_iou[on] = self.counts[on, 0].astype(np.float64) / self.counts[on, 1].astype(np.float64)
        self.video_iou = float("nan") if self.skipped else float(np.float64(self.counts[on, 0].sum()) / np.float64(self.counts[on, 1].sum()))

    def instance_iou(self):
        """-> float64 [F, P, A]: instance_actor_iou of the table."""
        return instance_actor_iou(self.table)


class PassScore:
    """A pass against truth.  result: the dict of evalmetrics.MapAccumulator.result() (the keys of EvalEngine.results()); videos: the
    VideoScore of every scored video in order; n_skipped: how many of them held no truth."""

    def __init__(self, result, videos):
        self.result, self.videos = result, list(videos)
        self.n_skipped = sum(1 for v in self.videos if v.skipped)


def score_pass(tables, labels, predicted, n_classes):
    """The host side of DetectEngine.score: per-video tables, true and predicted classes -> PassScore."""
    acc = evalmetrics.MapAccumulator(n_classes, device="cpu")
    videos = [VideoScore(t, l, p) for t, l, p in zip(tables, labels, predicted)]
    for v in videos:
        if not v.skipped:
            accumulate_video(v.counts, v.label, acc)
            acc.n_correct += int(v.correct)
    return PassScore(acc.result(), videos)


# ---------------------------------------------------------------------- a pass against truth at every mask threshold (tests/test_detect_sweep_cpu.py)
DEFAULT_SWEEP = tuple(k / 20.0 for k in range(1, 20))               # 0.05, 0.10 .. 0.95


def threshold_words(thresholds=None):
    """Mask thresholds t in (0, 1] (default: DEFAULT_SWEEP) -> words np.uint16 [N]: word = ceil(t * 65535), the product and its ceiling in
    float64; the mask at t is q >= word.  0.5 gives 32768, the word of a logit of +-0.0: the mask of that word is seg_positive's on every
    finite logit (include/picons.h, pc_frame_probs; csrc/evalpred.h).  The thresholds must ascend strictly and be at most
    ops.SWEEP_MAX_THRESHOLDS; ValueError for a t outside (0, 1], a NaN, too many, none, or two thresholds with one word."""
    try:
        t = np.asarray(DEFAULT_SWEEP if thresholds is None else thresholds, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("threshold_words: thresholds = %r are not numbers" % (thresholds,)) from None
    if t.ndim != 1 or not 1 <= t.size <= ops.SWEEP_MAX_THRESHOLDS:
        raise ValueError("threshold_words: 1..%d thresholds in one dimension, got shape %s" % (ops.SWEEP_MAX_THRESHOLDS, t.shape))
    if not (np.isfinite(t) & (t > 0.0) & (t <= 1.0)).all():
        raise ValueError("threshold_words: thresholds %s outside (0, 1]" % (t.tolist(),))
    words = np.ceil(t * float(ops.PROB_ONE)).astype(np.int64)
    if (np.diff(words) <= 0).any():
        raise ValueError("threshold_words: thresholds %s must ascend strictly and differ by at least one word of 1 / 65535 (words %s)"
                         % (t.tolist(), words.tolist()))
    return words.astype(np.uint16)


def cut_word(threshold):
    """One mask threshold in (0, 1] -> its word, an int in 1..65535: the one word of threshold_words([threshold]), with its refusals
    (ValueError).  The engine's word (DetectEngine.set_mask_threshold / recut) and the sweep's word are therefore the same function of the
    same float, and cut_word(w / 65535) == w for every word w: a word read off a SweepScore can be handed back as a threshold exactly."""
    return int(threshold_words([threshold])[0])


def _cut_threshold(who, threshold):
    """The (threshold, word) a video is cut at, or ValueError naming `who`: what cut_word refuses, and a bool."""
    if isinstance(threshold, (bool, np.bool_)):
        raise ValueError("%s: threshold = %r, a number in (0, 1]" % (who, threshold))
    try:
        word = cut_word(threshold)
    except ValueError as e:
        raise ValueError("%s: %s" % (who, e)) from None
    return float(threshold), word


def sweep_counts(hist):
    """Histograms int32 [F, 2, N + 1] of pc_prob_truth_hist -> int64 [N, F, 3]: per threshold k the (inter, union, gt) of crosstab_counts for
    the mask q >= word k.  A pixel is positive at k exactly if more than k words are at or below it, so inter_k = sum(hist[f, 1, k + 1:]),
    gt = sum(hist[f, 1, :]), union_k = gt + sum(hist[f, 0, k + 1:])."""
    h = np.asarray(hist).astype(np.int64)
    if h.ndim != 3 or h.shape[1] != 2 or h.shape[2] < 2:
        raise ValueError("sweep_counts: histograms [F, 2, N + 1], got %s" % (h.shape,))
    above = np.cumsum(h[:, :, ::-1], axis=2)[:, :, ::-1]               # above[f, t, b] = sum(h[f, t, b:])
    out = np.empty((h.shape[2] - 1, h.shape[0], 3), np.int64)
    out[:, :, 0] = above[:, 1, 1:].T
    out[:, :, 2] = above[:, 1, 0][None, :]
    out[:, :, 1] = out[:, :, 2] + above[:, 0, 1:].T
    return out


class SweepScore:
    """A pass against truth at N mask thresholds.  thresholds float64 [N] and words uint16 [N] (threshold_words); results: per threshold the
    dict of evalmetrics.MapAccumulator.result() -- PassScore.result, had the masks been cut at that word; fmAP / vmAP float64 [N, 20]: their
    rows, one column per IoU threshold 0, 0.05 .. 0.95; pixel int64 [N, 3] = (tp, fp, fn) over every frame of every scored video; videos: the
    histogram int32 [F, 2, N + 1] of every video of the call in order, skipped ones included; n_skipped: how many held no truth."""

    def __init__(self, thresholds, words, results, pixel, videos, n_skipped):
        self.thresholds, self.words = np.asarray(thresholds, np.float64), np.asarray(words, np.uint16)
        self.results, self.videos, self.n_skipped = list(results), list(videos), int(n_skipped)
        self.fmAP = np.array([r["fmAP"] for r in self.results], np.float64).reshape(len(self.results), -1)
        self.vmAP = np.array([r["vmAP"] for r in self.results], np.float64).reshape(len(self.results), -1)
        self.pixel = np.asarray(pixel, np.int64).reshape(len(self.results), 3)

    def best(self, metric="fmAP", iou=0.5):
        """The index of the first threshold at which `metric` ("fmAP" or "vmAP") at the IoU threshold `iou` (a multiple of 0.05 in
        [0, 0.95]) is largest; NaN (no scored video of some class) is ignored, ValueError if every value is NaN."""
        if metric not in ("fmAP", "vmAP"):
            raise ValueError("best: metric = %r, \"fmAP\" or \"vmAP\"" % (metric,))
        try:
            col = int(round(float(iou) * 20.0))
        except (TypeError, ValueError):
            raise ValueError("best: iou = %r is not a number" % (iou,)) from None
        if not 0 <= col < evalmetrics.N_THR or abs(float(iou) * 20.0 - col) > 1e-9:
            raise ValueError("best: iou = %r, a multiple of 0.05 in [0, 0.95]" % (iou,))
        v = getattr(self, metric)[:, col]
        if v.size == 0 or np.isnan(v).all():
            raise ValueError("best: %s at IoU %.2f is NaN at every threshold" % (metric, col / 20.0))
        return int(np.nanargmax(v))


def sweep_pass(hists, labels, predicted, n_classes, words, thresholds=None):
    """The host side of DetectEngine.sweep: per-video histograms [F, 2, N + 1], true and predicted classes, the N words they were split by
    (and the thresholds behind them: words / 65535 when None) -> SweepScore.  Threshold k's counts of every video go through accumulate_video
    into a MapAccumulator of its own; a video without a truth pixel enters none of them, as in score_pass."""
    words = np.asarray(words).reshape(-1)
    N = int(words.size)
    hists = [np.asarray(h) for h in hists]
    counts = [sweep_counts(h) for h in hists]
    for c in counts:
        if c.shape[0] != N:
            raise ValueError("sweep_pass: a histogram of %d thresholds for %d words" % (c.shape[0], N))
    accs = [evalmetrics.MapAccumulator(n_classes, device="cpu") for _ in range(N)]
    pixel = np.zeros((N, 3), np.int64)
    n_skipped = 0
    for c, label, pred in zip(counts, labels, predicted):
        if not (c[0, :, 2] != 0).any():                               # gt is the same at every threshold
            n_skipped += 1
            continue
        for k in range(N):
            accumulate_video(c[k], label, accs[k])
            accs[k].n_correct += int(int(label) == int(pred))
        inter, union, gt = (c[:, :, j].sum(axis=1) for j in range(3))
        pixel += np.stack([inter, union - gt, gt - inter], axis=1)    # pred = inter + fp, union = gt + fp
    t = words.astype(np.float64) / float(ops.PROB_ONE) if thresholds is None else thresholds
    return SweepScore(t, words, [a.result() for a in accs], pixel, hists, n_skipped)


def check_instances(instances, min_area, conn, masks):
    """The instance arguments of DetectEngine -> (K, min_area, conn) as ints, or ValueError."""
    K, min_area, conn = int(instances), int(min_area), int(conn)
    if not 0 <= K <= ops.INST_MAX_K or min_area < 1 or conn not in (4, 8):
        raise ValueError("DetectEngine: instances = %d (0..%d), min_area = %d (>= 1), conn = %d (4 or 8)" % (K, ops.INST_MAX_K, min_area, conn))
    if K > 0 and not masks:
        raise ValueError("DetectEngine: instances = %d needs masks=True (pc_frame_instances reads the masks)" % K)
    return K, min_area, conn


def substitute_overflow(counts, boxes, min_area, inst):
    """The instance fields of a video with the frames whose overflow flag is set holding one instance, the frame's own count and box."""
    n, kept, flags, areas, ibox, first = inst
    for f in np.flatnonzero(flags & 1).tolist():
        one = int(counts[f] >= min_area)
        n[f] = kept[f] = one
        if one:
            areas[f, 0], ibox[f, 0], first[f, 0] = counts[f], boxes[f], -1
    return n, kept, flags, areas, ibox, first


def score_instances(sums, npix, kept, flags):
    """The decoded pc_instance_scores record of a video (sums int64 [F, K + 1], npix int32 [F, K + 1]) and its instance fields AFTER
    substitute_overflow -> (inst_scores float64 [F, K], other_score float64 [F]): sum / (65535 * npix) for the ranks below kept, 0 from there
    on; slot K's mean, 0 when it is empty.  A frame with the overflow flag holds all its foreground in slot K (its map is 255 throughout):
    its one substituted instance takes that score."""
    sums, npix = np.asarray(sums, np.int64), np.asarray(npix, np.int64)
    F, K = sums.shape[0], sums.shape[1] - 1
    mean = np.where(npix > 0, sums.astype(np.float64) / (float(ops.PROB_ONE) * np.maximum(npix, 1)), 0.0)
    inst_scores, other = mean[:, :K].copy(), mean[:, K].copy()
    kept = np.asarray(kept).reshape(F)
    inst_scores[np.arange(K)[None, :] >= kept[:, None]] = 0.0
    for f in np.flatnonzero(np.asarray(flags).reshape(F) & 1).tolist():
        if kept[f]:
            inst_scores[f, 0] = other[f]
    return inst_scores, other


def collect_launches(n, V, slot, first, row0, per):
    """The launches (32 clips at most each) that collect a segment of n clips and V views behind its forward.  The segment begins at batch
    slot `slot` with the video's clip `first`, view v of its clip c at slot v * n + c; a slot holds `per` logits; row0: the video's first
    score row.  -> [(lo, hi, s0, s1, row)]: the logits [lo:hi] of clips [s0:s1] of the video at view stride n, `row` the first one's row."""
    return [((slot + q) * per, (slot + q + (V - 1) * n + min(32, n - q)) * per, first + q, first + q + min(32, n - q), row0 + (first + q) * V)
            for q in range(0, n, 32)]


def record_layout(F, C, K, scores, links):
    """The words of a video's device record, in the order one copy takes them to the host -> a namespace of slices: rec (F records of 8
    words), cls (the class vector, C + 2), inst (F instance records of 4 + 6K words, K > 0), score (F * 3 (K + 1) words with instance scores),
    link (F * links * (K + 1)^2 words); words: their total.  A part that is not asked for is empty and moves nothing in front of it."""
    sizes = dict(rec=F * ops.DETECT_REC_WORDS, cls=C + 2, inst=F * (ops.INST_HDR + K * ops.INST_WORDS) if K else 0,
                 score=F * ops.SCORE_WORDS * (K + 1) if scores else 0, link=F * links * (K + 1) ** 2)
    lay = SimpleNamespace(words=0)
    for name, words in sizes.items():
        setattr(lay, name, slice(lay.words, lay.words + words))
        lay.words += words
    return lay


class DetectEngine(ClipEngine):
    """Detects with the weights in the flat buffers P, R: a StepEngine's own (StepEngine.detect_engine: no copy, behind its lanes) or, built
    from a state dict, buffers of its own (load_state per checkpoint).

    begin() once per pass, add_video(frames_u8) per video, results() at the end -- or detect(frames_u8).  pack as in EvalEngine.
    masks=False: records only (the kernel gets a null mask).

    tile / flip: make_views per video (every frame pixel covered; each crop also mirrored); views: an explicit list of (h0, w0, flip) for
    every video.  With any of the three the engine runs V views per clip: all V share a batch, so a batch holds bs // V clips -- bs should be
    a multiple of V, bs < V is refused -- and a video takes clips * V rows of the score ring, row0 + clip * V + view, over all of which its
    class is voted.  A segment of n clips lies view-major in the batch (view v of its clip c at slot v * n + c of the segment's n * V slots:
    the order on_batch / outputs() show).  Without them: the centre crop, cut as the one view (h0, w0, 0), and pc_detect_frames.

    instances=K > 0 (at most 32; needs masks): behind a video's last clip ONE pc_frame_instances launch over all its frames splits every mask
    into its connected components (conn 4 or 8) of at least min_area pixels and leaves the K largest per frame behind the class vector, so
    the one copy to the host takes them too; instance_maps=True also keeps the map of ranks on the device (Detection.imap).  instances=0:
    nothing of this, today's path and buffer sizes.

    instance_scores=True (needs instances > 0): one pc_frame_probs launch behind every pc_detect_frames* keeps the per-pixel probability of
    the video (16-bit [F,H,W], Detection.probs), one pc_instance_scores launch behind pc_frame_instances reduces it per instance into
    F * 3 * (K + 1) words behind the instance records: Detection.inst_scores / other_score.  The map of ranks is then made whether or not
    instance_maps asks for it.  False: nothing of this, no buffer and no launch.

    instance_links=L in 1..4 (needs instances > 0): one pc_instance_overlaps launch behind pc_frame_instances counts, for every frame and
    each of the L frame distances, the pixels every instance shares with every instance of the later frame, into F * L * (K + 1)^2 words
    behind the score words: Detection.inst_overlaps, and with it instance_tubes(link="mask").  The map of ranks is then made whether or not
    instance_maps asks for it.  0: nothing of this, no buffer and no launch.

    set_working_frame((Hs, Ws), interpolation): videos added from then on are resized on the device to Hs x Ws, cut and run there, and
    detected at native size through pc_detect_frames_scaled (below).

    set_clip_hop(hop): videos added from then on are cut into overlapping windows that start every `hop` frames and every frame is
    detected from the mean of the windows that hold it (below).

    set_keep_probs(True): videos added from then on keep their probability map (Detection.probs) without instances; sweep(truths, labels)
    then scores the pass at every mask threshold from one histogram launch per video (below).

    set_mask_threshold(t): videos added from then on keep their probability map and are cut at the word cut_word(t) by one pc_prob_cut
    launch behind their last clip, in front of the class vote and the instances (below).  recut(t), after results(): the finished pass cut
    again at t on the device, with no second forward (below)."""

    mask_threshold = None                # set_mask_threshold: (threshold, word) for the videos to come, None for seg_positive's mask
    ws_cut = None                        # pc_prob_cut's partials, grown only for a larger video
    hop = None                           # set_clip_hop: the distance between two windows for the videos to come, None for today's cut
    ws_planes = None                     # pc_detect_frames_planes' partials, grown only for a larger frame

    def __init__(self, bs=14, hw=224, num_classes=24, device="cuda:0", state=None, engine=None, capacity=256, seed=47, f_skip=2, pack=False,
                 masks=True, on_batch=None, tile=False, flip=False, views=None, instances=0, min_area=1, conn=8, instance_maps=False,
                 instance_scores=False, instance_links=0):
        hw = engine.hw if engine is not None else hw
        self.inst_k, self.min_area, self.conn = check_instances(instances, min_area, conn, masks)
        self.instance_maps = bool(instance_maps) and self.inst_k > 0
        self.instance_scores = bool(instance_scores)
        if self.instance_scores and self.inst_k == 0:
            raise ValueError("DetectEngine: instance_scores=True needs instances > 0 (the scores are reduced over pc_frame_instances' map of ranks)")
        self.instance_links = int(instance_links)
        if not 0 <= self.instance_links <= ops.LINK_MAX_LAGS:
            raise ValueError("DetectEngine: instance_links = %d outside 0..%d" % (self.instance_links, ops.LINK_MAX_LAGS))
        if self.instance_links and self.inst_k == 0:
            raise ValueError("DetectEngine: instance_links = %d needs instances > 0 (the overlaps are counted over pc_frame_instances' map of ranks)"
                             % self.instance_links)
        if hw % 4:
            raise ValueError("DetectEngine: hw = %d must be a multiple of 4 (pc_detect_frames reads the logit rows 16 bytes at a time)" % hw)
        self._setup(bs, hw, num_classes, device, state, engine, capacity, seed, f_skip, pack, on_batch)
        self.masks = bool(masks)
        self.tile, self.flip, self.view_list = bool(tile), bool(flip), (None if views is None else list(views))
        self.multi = self.tile or self.flip or views is not None
        self.ws = torch.empty(ops.detect_frames_ws_bytes(min(bs, 32), self.hw), dtype=torch.uint8, device=self.dev)
        self.ws_views = None                 # the merge's partials: sized for the first video's frame, grown only for a larger one
        self.work = None                     # set_working_frame: (Hs, Ws, interpolation) for the videos to come, None for the video's own scale
        self.ws_scaled = None                # pc_detect_frames_scaled's partials and merged plane, grown only for a larger video
        self.pins = []                       # page-locked chunks the records of a pass are copied into
        # upload staging: two page-locked slots, so that the host fills one while the copy stream still reads the other (EvalEngine has one:
        # it waits for every video's flags).  A slot is filled again once the upload of two videos ago has left it.
        self.up_pin, self.up_done, self.up_slot = [None, None], [None, None], 0
        self.run_pins = [None, None]         # page-locked staging of mask_runs: per-frame offsets, runs
        # score: two page-locked slots the truths go up through (as up_pin), the tables' staging and the kernel's workspace; all made by the first call
        self.tr_pin, self.tr_done, self.tr_slot = [None, None], [None, None], 0
        self.score_pin = self.score_ws = None
        self.bx_pin, self.bx_done, self.bx_slot = [None, None], [None, None], 0       # box truths: a pair of slots all rect tables of a call go up through, in one copy
        self.keep_probs = False              # set_keep_probs: the probability map of the videos to come without instance scores
        self.sweep_pin = self.sweep_ws = None        # sweep: the histograms' staging and the kernel's workspace, made by the first call
        self._clear()

    def _clear(self):
        self.videos = []                     # the pass's videos in arrival order
        self.pin_i = self.pin_off = 0

    def _stage(self, words):
        """`words` int32 of page-locked memory, this pass's own until the next begin()."""
        while self.pin_i < len(self.pins) and self.pin_off + words > self.pins[self.pin_i].numel():
            self.pin_i, self.pin_off = self.pin_i + 1, 0
        if self.pin_i == len(self.pins):
            self.pins.append(torch.empty(max(words, PIN_CHUNK_WORDS), dtype=torch.int32).pin_memory())
        o = self.pin_off
        self.pin_off += words
        return self.pins[self.pin_i][o:o + words]

    def set_working_frame(self, size=None, interpolation="area"):
        """size = (Hs, Ws), ints of at least hw: every video added from now on is resized on the device to Hs x Ws with cv2.resize's
        arithmetic (interpolation "nearest", "linear" or "area": one pc_resize_u8 per video on the compute stream, skipped when the video has
        that size already), its views are crops of that working frame -- so a video smaller than hw, or one whose tiles at its own scale
        would be too many, can be taken -- and one pc_detect_frames_scaled launch per video segment merges the views on the working frame and
        resamples the merged logits bilinearly to every native pixel in front of the threshold, the box, the score and the probability
        map.  Masks, maps of ranks, probabilities, boxes and instances stay native [F, H, W]; Detection.views are in working coordinates
        and Detection.work = (Hs, Ws, interpolation).  Each video keeps the working size it was added under.  size=None: the video's own
        scale again, today's launches.  ValueError for anything else; nothing changes then."""
        if size is None:
            self.work = None
            return
        try:
            Hs, Ws = size
        except (TypeError, ValueError):
            raise ValueError("set_working_frame: size = %r, (Hs, Ws) or None" % (size,)) from None
        for v in (Hs, Ws):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("set_working_frame: size = %r, two ints" % (size,))
        Hs, Ws = int(Hs), int(Ws)
        if Hs < self.hw or Ws < self.hw or Hs * Ws >= 1 << 31:
            raise ValueError("set_working_frame: a working frame of %d x %d is smaller than the %d x %d crop (or holds 2^31 pixels)" % (Hs, Ws, self.hw, self.hw))
        if not isinstance(interpolation, str) or interpolation not in INTERPOLATIONS:
            raise ValueError("set_working_frame: interpolation = %r, one of %s" % (interpolation, ", ".join(sorted(INTERPOLATIONS))))
        self.work = (Hs, Ws, interpolation)

    def set_clip_hop(self, hop=None):
        """hop: an int, a multiple of f_skip in [f_skip, 8 * f_skip): every video added from now on is cut into windows of 8 * f_skip frames
        that start every `hop` frames (clip_starts_hop), so a frame lies in up to ceil(8 * f_skip / hop) clips.  Behind each forward one
        pc_clip_planes launch per video segment (instead of pc_detect_frames* and pc_frame_probs) keeps the merged logits of the clips'
        frames in the video's slot planes -- M * F * pstride * 4 + pstride bytes, M = ceil(8 * f_skip / hop), pstride the pixels of the
        frame the views are cut from rounded up to 4, held until the video's last clip has run --, and behind that clip
        pc_detect_frames_planes averages per frame the windows that hold it, in window order, in front of the resample (the identity
        without a working frame), the threshold, the box, the score and the probability.  Masks, records, instances, scores, links, runs and
        score() are made from that as before; the class is voted over the rows of ALL the video's clips, which now overlap.  Each video
        keeps the hop it was added under (Detection.hop).  hop=None or 8 * f_skip: today's cut and today's launches.  ValueError for
        anything else; nothing changes then."""
        span = 8 * self.f_skip
        if hop is None:
            self.hop = None
            return
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)):
            raise ValueError("set_clip_hop: hop = %r, an int or None" % (hop,))
        hop = int(hop)
        if hop % self.f_skip or not self.f_skip <= hop <= span:
            raise ValueError("set_clip_hop: hop = %d, a multiple of f_skip = %d in [%d, %d]" % (hop, self.f_skip, self.f_skip, span))
        self.hop = None if hop == span else hop

    def set_keep_probs(self, keep=True):
        """keep=True: every video added from now on keeps its per-pixel probability map on the device (Detection.probs, 16-bit [F,H,W] in
        steps of 1 / 65535) whether or not the engine reduces it per instance: one pc_frame_probs launch behind each pc_detect_frames /
        pc_detect_frames_views, the prob operand of pc_detect_frames_scaled / pc_detect_frames_planes -- what instance_scores=True keeps
        already, without instances -- and with it sweep().  keep=False: only what instance_scores asks for, today's launches.  A bool
        only: ValueError for anything else; nothing changes then."""
        if not isinstance(keep, (bool, np.bool_)):
            raise ValueError("set_keep_probs: keep = %r, True or False" % (keep,))
        self.keep_probs = bool(keep)

    def set_mask_threshold(self, threshold=None):
        """threshold: a number in (0, 1].  Every video added from now on is cut at the word cut_word(threshold) -- the word sweep() gives
        that threshold -- instead of at seg_positive's sigmoid(x) >= 0.5: the video keeps its probability map whether or not keep_probs /
        instance_scores ask for it (filled by the route's own launches, as under set_keep_probs(True)), and behind its last clip ONE
        pc_prob_cut launch over all its frames rewrites its mask (q >= word) and words 0..5 of its records (count, box, score) -- behind the
        hop path's pc_detect_frames_planes, in front of pc_video_class, pc_frame_instances, the instance scores and the overlaps, which run
        on that mask unchanged.  The existing detect kernels are not told the threshold: the price is one more pass over the map.  Each
        video keeps the threshold it was added under (Detection.threshold = (threshold, word)); its frame_scores are means of probability
        words (Detection).  threshold=None: seg_positive's mask again, today's launches and nothing else.  ValueError for anything
        threshold_words refuses and for a bool; nothing changes then."""
        self.mask_threshold = None if threshold is None else _cut_threshold("set_mask_threshold", threshold)

    def _grow(self, name, n, pin=None, slot=None):
        """The engine's buffer `name` (element `slot` of it, where it is a pair) with room for n elements -> the buffer: None until first
        needed, made then, made anew only for a larger n.  pin=None: uint8 on the device, a kernel's workspace; else page-locked host memory
        of dtype `pin`, 1024 elements at least."""
        buf = getattr(self, name) if slot is None else getattr(self, name)[slot]
        if buf is None or buf.numel() < n:
            buf = torch.empty(n, dtype=torch.uint8, device=self.dev) if pin is None else torch.empty(max(n, 1024), dtype=pin).pin_memory()
            if slot is None:
                setattr(self, name, buf)
            else:
                getattr(self, name)[slot] = buf
        return buf

    def _frame(self, H, W):
        """The frame the views of an H x W video are cut from: the working frame if one is set, else its own."""
        return (H, W) if self.work is None else self.work[:2]

    # ------------------------------------------------------------------ the pass
    def check_video(self, frames):
        """Refuse (ValueError) a video the engine cannot take, before anything is enqueued or changed.  -> (frames, clip starts, row0, next row)."""
        v = _as_u8(frames, "frames")
        if v.dim() != 4 or v.shape[3] != 3 or v.shape[0] < 1:
            raise ValueError("frames: shape %s, expected (F, H, W, 3)" % (tuple(v.shape),))
        F, H, W = (int(s) for s in v.shape[:3])
        if self.work is None and (H < self.hw or W < self.hw):
            raise ValueError("frames of %d x %d are smaller than the %d x %d crop" % (H, W, self.hw, self.hw))
        if self.work is not None and (H < 1 or W < 1 or ops.detect_frames_scaled_ws_bytes(1, self.work[0], self.work[1], H, W) < 0):
            raise ValueError("frames of %d x %d cannot be resampled from a working frame of %d x %d" % ((H, W) + self.work[:2]))
        width = len(self.video_views(*self._frame(H, W)) or (0,))
        if self.hop is None:
            starts = clip_starts(F, np.ones(F, np.int32), self.f_skip)    # every clip with a real frame: each frame belongs to exactly one
        else:
            starts = clip_starts_hop(F, self.f_skip, self.hop)            # overlapping windows: a frame belongs to up to ceil(span / hop) clips
            if len(starts) * width > self.capacity - self.bs:
                raise ValueError("a video of %d frames takes %d clips at hop = %d, %d rows of the tables: more than capacity - bs = %d - %d"
                                 % (F, len(starts), self.hop, len(starts) * width, self.capacity, self.bs))
            if ops.clip_planes_bytes(F, *self._frame(H, W), self.f_skip, self.hop) < 0 or ops.detect_frames_planes_ws_bytes(1, H, W) < 0:
                raise ValueError("frames of %d x %d cannot be detected at hop = %d" % (H, W, self.hop))
        row0, pos = ring_place(self.pos, len(starts) * width, self.capacity, self.bs)
        return v, starts, row0, pos

    def video_views(self, H, W):
        """The views of a video cut from H x W frames (its working frame, if one is set), None for the centre crop alone.  ValueError for
        views the engine cannot take."""
        if not self.multi:
            return None
        views = make_views(H, W, self.hw, self.tile, self.flip) if self.view_list is None else check_views(self.view_list, H, W, self.hw)
        if len(views) > self.bs:
            raise ValueError("frames of %d x %d take %d views per clip, more than the bs = %d clips of a batch" % (H, W, len(views), self.bs))
        return views

    def _width(self, rec):
        return len(rec.views)

    def add_video(self, frames_u8):
        """One video: frames [F,H,W,3] uint8 (numpy, host tensor or device tensor).  Uploaded through page-locked memory on the copy stream; its
        clips join the batches.  -> the index of the video in results()."""
        v, starts, row0, pos = self.check_video(frames_u8)
        F, H, W = (int(s) for s in v.shape[:3])
        frame = self._frame(H, W)                                     # crop and views: of the working frame, if one is set
        h0, w0 = centre_crop(*frame, self.hw)
        views = self.video_views(*frame)
        cut = views or [(h0, w0, 0)]                                  # the centre crop is the one view (h0, w0, 0)
        slot = self.up_slot
        self.up_slot ^= 1
        if self.up_done[slot] is not None:
            self.up_done[slot].synchronize()                          # an upload on the copy stream, two videos back: never the compute stream
        self.pin = self.up_pin[slot]
        dv, _none, entry = self._upload(v)
        self.up_pin[slot] = self.pin                                  # (grown, if the video was larger than the slot)
        rec = SimpleNamespace(video=dv, truth=None, entry=entry, F=F, H=H, W=W, h0=h0, w0=w0, ready=torch.cuda.Event(), waited=False,
                              starts=starts, rows=len(starts) * len(cut), done=0, views=cut, centre=views is None, frame=frame, work=self.work,
                              wvideo=None)
        rec.ready.record(self.copy_stream)
        self.up_done[slot] = rec.ready
        # records, class vector and what instances add side by side: one copy to the host takes them all.  Every frame below F belongs to a
        # clip, so every mask byte and every record is written by a launch: nothing is filled.
        rec.at = record_layout(F, self.C, self.inst_k, self.instance_scores, self.instance_links)
        rec.score_words, rec.link_words = (s.stop - s.start for s in (rec.at.score, rec.at.link))
        rec.dev = torch.empty(rec.at.words, dtype=torch.int32, device=self.dev)
        rec.mask = torch.empty(F, H, W, dtype=torch.uint8, device=self.dev) if self.masks else None
        rec.imap = torch.empty(F, H, W, dtype=torch.uint8, device=self.dev) if self.instance_maps or self.instance_scores or self.instance_links else None
        rec.prob = torch.empty(F, H, W, dtype=torch.int16, device=self.dev) if self.instance_scores or self.keep_probs or self.mask_threshold else None
        rec.pin = None
        rec.cut = self.mask_threshold
        if rec.cut:
            self._grow("ws_cut", ops.prob_cut_ws_bytes(F, H, W))
        rec.hop, rec.planes = self.hop, None
        if rec.hop:
            # the slot planes and the cover of the frame the views are cut from, in one allocation, until the video's last clip has run;
            # every (slot, frame) that is read has been written by a launch: nothing is filled
            rec.planes = torch.empty(ops.clip_planes_bytes(F, *frame, self.f_skip, rec.hop), dtype=torch.uint8, device=self.dev)
            self._grow("ws_planes", ops.detect_frames_planes_ws_bytes(min(F, ops.PLANES_MAX_FRAMES), H, W))
        elif rec.work:
            self._grow("ws_scaled", ops.detect_frames_scaled_ws_bytes(min(self.bs // len(cut), 32), *frame, H, W))
        elif views:
            self._grow("ws_views", ops.detect_frames_views_ws_bytes(min(self.bs, 32), H, W))
        self.videos.append(rec)
        self._join(rec, row0, pos)
        return len(self.videos) - 1

    def _cut(self, rec, first, k, slot, seg):
        # view v of the segment's clip c at slot v * seg + c: this launch's clips start at `slot`.  The centre crop is the one view at stride seg.
        per, views = self.per, rec.views
        video = rec.video
        if rec.work:
            if rec.wvideo is None:                                    # the video's first cut, behind rec.ready on this stream: its one resize
                Hs, Ws, interp = rec.work
                rec.wvideo = video if (Hs, Ws) == (rec.H, rec.W) else ops.resize_u8(video, Hs, Ws, INTERPOLATIONS[interp])
            video = rec.wvideo
        ops.clips_from_u8_views(video, views, self.hw, rec.starts[first:first + k], self.f_skip, view_stride=seg,
                                out=self.img[slot * per * 4:(slot + (len(views) - 1) * seg + k) * per * 4])

    def _release(self, v):
        super()._release(v)
        v.wvideo = None                                               # made and read on the compute stream alone

    def _collect(self, rec, first, n, slot):
        F, H, W, (Hs, Ws), views, fs = rec.F, rec.H, rec.W, rec.frame, rec.views, self.f_skip
        out = dict(mask=rec.mask, rec=rec.dev[rec.at.rec].view(F, -1), want_mask=False)
        for lo, hi, s0, s1, row in collect_launches(n, len(views), slot, first, rec.row0, self.per):
            logits, starts = self.out[lo:hi].view(-1, 8, self.hw, self.hw), rec.starts[s0:s1]
            if rec.hop:
                # the views merged on the frame they are cut from, into the video's slot planes; the cover bytes with the video's first
                # launch.  Mask, records and probability wait for the last clip (_finish).
                ops.clip_planes(logits, views, starts, F, Hs, Ws, fs, rec.hop, view_stride=n, planes=rec.planes, cover=s0 == 0)
            elif rec.work:
                # the views merged on the working frame, resampled to native size, and the probability map with them
                ops.detect_frames_scaled(logits, views, starts, F, H, W, Hs, Ws, fs, view_stride=n, row0=row, prob=rec.prob, ws=self.ws_scaled, **out)
            else:
                if rec.centre:
                    ops.detect_frames(logits, starts, F, H, W, rec.h0, rec.w0, fs, row0=row, ws=self.ws, **out)
                else:
                    ops.detect_frames_views(logits, views, starts, F, H, W, fs, view_stride=n, row0=row, ws=self.ws_views, **out)
                if rec.prob is not None:
                    ops.frame_probs(logits, views, starts, F, H, W, fs, view_stride=n, prob=rec.prob)

    def _finish(self, rec):
        """The video's class from its score rows, its instances from its masks (every frame has been written by now, on this stream); records,
        class vector and instances on their way to the host."""
        at = rec.at
        if rec.hop:
            # every clip's frames lie in the slot planes: per frame the mean of the windows that hold it -> mask, probability and records
            for f0 in range(0, rec.F, ops.PLANES_MAX_FRAMES):
                ops.detect_frames_planes(rec.planes, rec.F, rec.H, rec.W, *rec.frame, self._width(rec), self.f_skip, rec.hop, f0,
                                         min(ops.PLANES_MAX_FRAMES, rec.F - f0), row0=rec.row0, mask=rec.mask, prob=rec.prob,
                                         rec=rec.dev[at.rec].view(rec.F, -1), ws=self.ws_planes, want_mask=False)
            rec.planes = None                                         # written and read on the compute stream alone: the allocator may reuse them
        if rec.cut:
            # the kept probability map, whole by now, cut at the video's word: mask and words 0..5 of the records anew
            ops.prob_cut(rec.prob, rec.cut[1], mask=rec.mask, rec=rec.dev[at.rec].view(rec.F, -1), ws=self.ws_cut, want_mask=False)
        ops.video_class(self.scores[rec.row0:rec.row0 + rec.rows], out=rec.dev[at.cls].view(torch.float32))
        self._instances(rec)
        self._to_host(rec)

    def _to_host(self, rec):
        """The video's record into page-locked memory of its own, the copy enqueued behind the launches that wrote it."""
        rec.pin = self._stage(rec.dev.numel())
        rec.pin.copy_(rec.dev, non_blocking=True)

    def _predicted(self, rec):
        """The class vector of the video's staged record (rec.pin, copied by now) -> (label, class_score, class_scores [C]), copies."""
        cls = rec.pin.numpy()[rec.at.cls].copy().view(np.float32)
        return int(cls[self.C]), float(cls[self.C + 1]), cls[:self.C].copy()

    def _instances(self, rec):
        """The video's instances, their scores and their overlaps from its mask, into their words of rec.dev and into rec.imap."""
        at = rec.at
        if self.inst_k:
            ops.frame_instances(rec.mask, conn=self.conn, min_area=self.min_area, K=self.inst_k, inst=rec.dev[at.inst].view(rec.F, -1), imap=rec.imap,
                                want_imap=False)
            if self.instance_scores:
                ops.instance_scores(rec.imap, rec.prob, self.inst_k, out=rec.dev[at.score].view(rec.F, -1))
            if self.instance_links:
                ops.instance_overlaps(rec.imap, self.inst_k, self.instance_links, out=rec.dev[at.link])

    def _detection(self, rec):
        """The video's staged record (rec.pin, copied by now) -> its Detection."""
        words, at = rec.pin.numpy(), rec.at
        counts, boxes, fscores, _rows = ops.decode_detect_records(words[at.rec])
        inst = scores = overlaps = None
        if self.inst_k:
            n, kept, _runs, flags, areas, ibox, first = ops.decode_instances(words[at.inst], self.inst_k)
            inst = substitute_overflow(counts, boxes, self.min_area, (n, kept, flags, areas, ibox, first))
            if self.instance_scores:
                sums, npix = ops.decode_instance_scores(words[at.score], self.inst_k)
                scores = score_instances(sums, npix, inst[1], inst[2])
            if self.instance_links:
                overlaps = ops.decode_instance_overlaps(words[at.link], self.inst_k, self.instance_links)
        d = Detection(*self._predicted(rec), counts, boxes, fscores, rec.mask, list(rec.views), inst, rec.imap if self.instance_maps else None, scores,
                      rec.prob, overlaps)
        if rec.work:
            d.work = tuple(rec.work)
        if rec.hop:
            d.hop = rec.hop
        if rec.cut:
            d.threshold = tuple(rec.cut)
        return d

    def results(self):
        """The pass's one host wait -> [Detection], one per video in arrival order."""
        self.flush()
        torch.cuda.current_stream(self.dev).synchronize()
        return [self._detection(rec) for rec in self.videos]

    def recut(self, threshold, videos=None):
        """The last pass cut again at `threshold` (a number in (0, 1]: the word cut_word(threshold), the one sweep() gives it) -> [Detection],
        one per video in arrival order, or per index in `videos`.  Called after results() -- the natural step after sweep().best() -- and
        again with another threshold; no forward runs.  Per picked video, on the compute stream: pc_prob_cut over its kept probability map
        into its mask (null with masks=False) and words 0..5 of its records; pc_frame_instances / pc_instance_scores / pc_instance_overlaps
        into their words and into the map of ranks, as behind a video's last clip, when the engine has instances; the whole record to fresh
        page-locked staging.  ONE host wait per call, however many videos.

        recut works IN PLACE ON THE DEVICE: the `masks` / `imap` tensors of Detection objects handed out earlier are the same tensors and
        show the new contents, their host arrays (counts, boxes, scores, instances) do not change; mask_runs(), score() and sweep() called
        afterwards see the re-cut pass.  Videos not picked are not touched.  Class label and scores, views, work, hop and probs are
        unchanged; Detection.threshold = (threshold, word), and frame_scores are means of probability words (Detection): recut(0.5) of a
        plain pass gives its masks, counts, boxes and instances bit for bit and its frame_scores within 1e-5.
        Every refusal is a ValueError before anything is enqueued or allocated: no finished pass, a threshold threshold_words refuses or a
        bool, an index outside the pass, a picked video that keeps no probability map."""
        self._check_pass("recut")
        cut = _cut_threshold("recut", threshold)
        picks = self._picks("recut", videos)
        for v in picks:
            if self.videos[v].prob is None:
                raise ValueError("recut: video %d keeps no probability map (set_keep_probs(True) or set_mask_threshold(t) before it is added, "
                                 "or instance_scores=True)" % v)
        if not picks:
            return []
        recs = [self.videos[v] for v in picks]
        for rec in recs:
            self._grow("ws_cut", ops.prob_cut_ws_bytes(rec.F, rec.H, rec.W))
        for rec in recs:
            ops.prob_cut(rec.prob, cut[1], mask=rec.mask, rec=rec.dev[rec.at.rec].view(rec.F, -1), ws=self.ws_cut, want_mask=False)
            self._instances(rec)
            rec.cut = cut
            self._to_host(rec)
        torch.cuda.current_stream(self.dev).synchronize()             # the call's one wait on the compute stream
        return [self._detection(rec) for rec in recs]

    def _check_pass(self, who):
        """The refusal everything that reads a pass (who) opens with: no finished pass."""
        if not self.videos or any(rec.pin is None for rec in self.videos):
            raise ValueError("%s: no finished pass (call it after results())" % who)

    def _check_which(self, who, which):
        """The refusal of mask_runs and score (who) in front of that: a `which` the engine does not keep."""
        if which not in ("masks", "imap"):
            raise ValueError("%s: which = %r, \"masks\" or \"imap\"" % (who, which))
        if which == "masks" and not self.masks:
            raise ValueError("%s: the engine keeps no masks (masks=False)" % who)
        if which == "imap" and not self.instance_maps:
            raise ValueError("%s: the engine keeps no maps of ranks (instances=K with instance_maps=True)" % who)

    def _picks(self, who, videos):
        """`videos` of mask_runs and score (who) -> the indices of the pass's videos they name, all of them for None."""
        picks = list(range(len(self.videos))) if videos is None else [int(v) for v in videos]
        for v in picks:
            if not 0 <= v < len(self.videos):
                raise ValueError("%s: video %d outside the %d of the pass" % (who, v, len(self.videos)))
        return picks

    def mask_runs(self, which="masks", videos=None):
        """The masks (which="masks") or the maps of ranks (which="imap": needs instance_maps=True) of the last pass as row runs -> [MaskRuns],
        one per video in arrival order, or per index in `videos`.  Called after results(); it changes nothing results() returned and can be
        called again.  Two host waits per call, however many videos: every video's runs are counted (pc_mask_run_index; a video of 2^31
        pixels or more in several frame ranges) and the per-frame offsets gathered into page-locked memory -- first wait --, then one buffer
        of exactly the pass's runs is filled (pc_mask_runs per range) and leaves in one asynchronous copy -- second wait.  Every refusal is a
        ValueError before anything is enqueued."""
        self._check_which("mask_runs", which)
        self._check_pass("mask_runs")
        picks = self._picks("mask_runs", videos)
        jobs = []                                                     # (map, f0, nf, first word of its offsets in the staging)
        words = 0
        for v in picks:
            rec = self.videos[v]
            if rec.F * rec.H > ops.RUN_MAX_ROWS:
                raise ValueError("mask_runs: video %d has %d rows, more than the 2^24 a run's row field numbers" % (v, rec.F * rec.H))
            for f0, nf in run_ranges(rec.F, rec.H, rec.W):
                jobs.append((rec.mask if which == "masks" else rec.imap, f0, nf, words))
                words += nf + 1
        stream = torch.cuda.current_stream(self.dev)
        # ---- phase 1: the index of every range; its entries at the frame starts and the total (index[::H]) to the host
        off_dev = torch.empty(words, dtype=torch.int32, device=self.dev)
        off_pin = self._grow("run_pins", words, torch.int32, 0)[:words]
        indexes = []
        for m, f0, nf, w0 in jobs:
            index = ops.mask_run_index(m, f0, nf)
            off_dev[w0:w0 + nf + 1] = index[::int(m.shape[1])]
            indexes.append(index)
        off_pin.copy_(off_dev, non_blocking=True)
        stream.synchronize()
        offs = off_pin.numpy().astype(np.int64)
        # ---- phase 2: one buffer of exactly the runs, filled range by range, one copy
        starts = np.zeros(len(jobs) + 1, np.int64)
        for j, (_m, _f0, nf, w0) in enumerate(jobs):
            starts[j + 1] = starts[j] + offs[w0 + nf]
        total = int(starts[-1])
        run_dev = torch.empty(total, ops.RUN_WORDS, dtype=torch.int32, device=self.dev)
        for j, (m, f0, nf, _w0) in enumerate(jobs):
            ops.mask_runs(m, indexes[j], f0, nf, runs=run_dev[int(starts[j]):int(starts[j + 1])])
        run_pin = self._grow("run_pins", total * ops.RUN_WORDS, torch.int32, 1)[:total * ops.RUN_WORDS]
        run_pin.copy_(run_dev.view(-1), non_blocking=True)
        stream.synchronize()
        words_host = run_pin.numpy().view(np.uint32).reshape(-1, ops.RUN_WORDS)
        out, j = [], 0
        for v in picks:
            rec = self.videos[v]
            ranges = run_ranges(rec.F, rec.H, rec.W)
            runs = words_host[int(starts[j]):int(starts[j + len(ranges)])].copy()          # the staging is used again by the next call
            offsets = np.zeros(rec.F + 1, np.int64)
            for k, (f0, nf) in enumerate(ranges):
                w0, lo = jobs[j + k][3], int(starts[j + k] - starts[j])
                offsets[f0 + 1:f0 + nf + 1] = lo + offs[w0 + 1:w0 + nf + 1]
                runs[lo:lo + int(offs[w0 + nf]), 0] += np.uint32(f0 * rec.H)                 # rows of the range -> rows of the video
            out.append(MaskRuns((rec.F, rec.H, rec.W), offsets, runs))
            j += len(ranges)
        return out

    def score(self, truths, labels, actors=1, which="masks", videos=None):
        """The last pass against truth masks -> PassScore.  truths[i]: uint8 [F,H,W] or [F,H,W,1] (numpy, host tensor or device tensor) for
        the i-th video of the pass, or of `videos`; any non-zero byte is truth, a byte 1..actors is that actor.  labels[i]: its class id.
        which="masks": the video's mask, P = 1; which="imap" (needs instance_maps=True): its map of ranks, P = K.  Called after results(); it
        changes nothing results() returned and can be called again.  Per video one upload through page-locked staging on the copy stream
        (the host waits at most for its own upload of two videos ago, never for the compute stream) and one pc_map_crosstab launch; all
        tables leave in one asynchronous copy and the call has ONE wait on the compute stream, after which the host does the rest
        (score_pass).  Unlike EvalEngine the truth is taken on the full frame, not inside the centre crop, and `correct` compares with the
        detection's class, voted over all clips of the video, where EvalEngine votes over the clips that hold truth.  Every refusal is a
        ValueError before anything is enqueued."""
        self._check_which("score", which)
        self._check_pass("score")
        try:
            A = int(actors)
        except (TypeError, ValueError):
            raise ValueError("score: actors = %r is not a number" % (actors,)) from None
        if A != actors or not 1 <= A <= ops.CROSS_MAX_SLOTS:
            raise ValueError("score: actors = %r outside 1..%d" % (actors, ops.CROSS_MAX_SLOTS))
        P = 1 if which == "masks" else self.inst_k

        def launch(rec, truth, out, ws):
            ops.map_crosstab(rec.mask if which == "masks" else rec.imap, truth, P, A, out=out.view(rec.F, P + 2, A + 2), ws=ws)
        tables, labs, predicted = self._truth_pass("score", truths, labels, videos, lambda rec: rec.F * (P + 2) * (A + 2),
                                                   lambda rec: ops.map_crosstab_ws_bytes(rec.F, rec.H, rec.W, P, A), launch,
                                                   lambda words: ops.decode_map_crosstab(words, P, A))
        return score_pass(tables, labs, predicted, self.C)

    def _truth_pass(self, who, truths, labels, videos, words_of, ws_of, launch, decode, check=None):
        """What score and sweep (who) do with the truths of a finished pass, once.  The refusals, in order -- an index outside the pass,
        not as many truths and labels as videos, then video by video: check(v, record), its truth, its label, the sizes ws_of(record)
        refuses -- in front of anything allocated or uploaded.  Then ONE buffer of words_of(record) int32 per video, the workspace
        `<who>_ws` grown to the largest ws_of(record) bytes, per video its truth uploaded and launch(record, truth on the device, its words,
        workspace) on the compute stream, all words in one asynchronous copy through the page-locked `<who>_pin`, and the call's one wait
        on the compute stream.  -> ([decode(words) per video]: copies, the staging is used again, [label], [predicted class])."""
        picks = self._picks(who, videos)
        truths, labels = check_counts(who, truths, labels, len(picks))
        jobs, labs, total, ws_need = [], [], 0, 0                       # (record, truth, its words in the buffer)
        for v, truth, label in zip(picks, truths, labels):
            rec = self.videos[v]
            if check:
                check(v, rec)
            t = check_truth(who, truth, rec.F, rec.H, rec.W, v)
            labs.append(check_label(who, label, self.C))
            jobs.append((rec, t, slice(total, total + words_of(rec))))
            total = jobs[-1][2].stop
            ws_need = max(ws_need, ws_of(rec))
        if not jobs:
            return [], [], []
        main = torch.cuda.current_stream(self.dev)
        ws = self._grow(who + "_ws", ws_need)
        tab_dev = torch.empty(total, dtype=torch.int32, device=self.dev)
        tables = self._box_tables([t for _rec, t, _at in jobs if isinstance(t, BoxTruth)], main)
        for rec, t, at in jobs:
            if isinstance(t, BoxTruth):                              # painted on the device with the rects' values (they carry the actors); the fresh map is written whole
                launch(rec, ops.paint_boxes(next(tables), *t.shape), tab_dev[at], ws)
            else:
                launch(rec, self._truth_to_device(t, main), tab_dev[at], ws)
        pin = self._grow(who + "_pin", total, torch.int32)[:total]
        pin.copy_(tab_dev, non_blocking=True)
        main.synchronize()                                           # the call's one wait on the compute stream
        host = pin.numpy()
        return [decode(host[at]) for _rec, _t, at in jobs], labs, [self._predicted(rec)[0] for rec, _t, _at in jobs]

    def sweep(self, truths, labels, thresholds=None, videos=None):
        """The last pass against truth masks at every mask threshold of `thresholds` (floats in (0, 1], ascending; default 0.05, 0.10 ..
        0.95: threshold_words) -> SweepScore: what score() would give had the masks been cut at each of them, from the probability maps the
        pass kept (set_keep_probs, or instance_scores=True).  truths, labels and videos as in score().  Called after results(); it changes
        nothing results() returned and can be called again.  Per video one upload of its truth (score()'s staging) and one
        pc_prob_truth_hist launch into its part of one buffer; all histograms leave in one asynchronous copy and the call has ONE wait on the
        compute stream, after which the host does the rest (sweep_pass).  Every refusal is a ValueError before anything is enqueued."""
        self._check_pass("sweep")
        t = np.asarray(DEFAULT_SWEEP, np.float64) if thresholds is None else thresholds
        words = threshold_words(t)
        t = np.asarray(t, np.float64)
        N = int(words.size)

        def keeps_prob(v, rec):
            if rec.prob is None:
                raise ValueError("sweep: video %d keeps no probability map (set_keep_probs(True) before it is added, or instance_scores=True)" % v)

        def launch(rec, truth, out, ws):
            ops.prob_truth_hist(rec.prob, truth, words, out=out.view(rec.F, 2, N + 1), ws=ws)
        hists, labs, predicted = self._truth_pass("sweep", truths, labels, videos, lambda rec: rec.F * 2 * (N + 1),
                                                  lambda rec: ops.prob_truth_hist_ws_bytes(rec.F, rec.H, rec.W, N), launch,
                                                  lambda h: ops.decode_prob_truth_hist(h, N), keeps_prob)
        return sweep_pass(hists, labs, predicted, self.C, words, t)

    def _truth_to_device(self, t, main):
        """A truth [F,H,W] on the device, contiguous, ordered in front of what `main` runs next.  A host truth goes through one of two
        page-locked slots on the copy stream; the host waits only for the upload that used the slot two truths ago."""
        if t.is_cuda:
            return t.to(self.dev).contiguous()
        slot = self.tr_slot
        self.tr_slot ^= 1
        if self.tr_done[slot] is not None:
            self.tr_done[slot].synchronize()                          # an upload on the copy stream: never the compute stream
        n = t.numel()
        if self.tr_pin[slot] is None or self.tr_pin[slot].numel() < n:
            self.tr_pin[slot] = torch.empty(n, dtype=torch.uint8).pin_memory()
        stage = self.tr_pin[slot][:n].view(t.shape)
        stage.copy_(t)
        with torch.cuda.stream(self.copy_stream):                    # allocated where it is written; the compute stream's use is recorded below
            d = torch.empty(t.shape, dtype=torch.uint8, device=self.dev)
            d.copy_(stage, non_blocking=True)
            self.tr_done[slot] = torch.cuda.Event()
            self.tr_done[slot].record(self.copy_stream)
        main.wait_event(self.tr_done[slot])
        d.record_stream(main)
        return d

    def _box_tables(self, truths, main):
        """The rect tables of a call's BoxTruths on the device, in order: all of them (F * R * 20 bytes each) through ONE page-locked slot of
        a pair of their own and ONE copy, in front of the paint launches on `main` -- per video nothing but its pc_paint_boxes launch is
        left.  The host waits only if the copy that used the slot two calls ago has not left it.  -> an iterator of int32 [F,R,5] tensors."""
        if not truths:
            return iter(())
        slot = self.bx_slot
        self.bx_slot ^= 1
        if self.bx_done[slot] is not None and not self.bx_done[slot].query():
            self.bx_done[slot].synchronize()
        words = sum(t.rects.size for t in truths)
        stage = self._grow("bx_pin", words, torch.int32, slot)[:words]
        host, at, o = stage.numpy(), [], 0
        for t in truths:
            host[o:o + t.rects.size] = t.rects.reshape(-1)
            at.append((o, t.rects.shape))
            o += t.rects.size
        dev = torch.empty(words, dtype=torch.int32, device=self.dev)
        dev.copy_(stage, non_blocking=True)
        self.bx_done[slot] = torch.cuda.Event()
        self.bx_done[slot].record(main)
        return (dev[o:o + int(np.prod(shape))].view(shape) for o, shape in at)

    def detect(self, frames_u8):
        """One video on its own: begin(), add_video, results()[0]."""
        self.begin()
        self.add_video(frames_u8)
        return self.results()[0]
