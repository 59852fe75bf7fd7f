"""The f-mAP / v-mAP evaluation on one MI355X from DECODED uint8 video: the reference's evaluate_ucf101.py:73-186 (evaluate_jhmdb.py: the
same loop, 21 classes) with the video uploaded as the decoder left it (uint8 frames, uint8 truth: 1/24 of the float64 the reference's loader
yields), the clips cut on the device straight into the tensor the stem reads (pc_eval_clips_from_u8, csrc/evalclips.hip), the eval forward
replayed from ONE op plan of `bs` clips whose weight layouts are made once per pass, and the per-frame counts, the per-class tables and the
class vote accumulated on the device (pc_seg_frame_counts, pc_map_accumulate, pc_video_vote).  One device-to-host copy per pass (`results`).

ClipEngine holds what EvalEngine shares with detect.DetectEngine (the inference side: unlabelled video in, masks, boxes and tubes out): the
plan, the upload pool, batch forming, the class-score ring and the batch itself.

The only host wait per video is for its F per-frame truth counts (pc_truth_frame_flags on the copy stream): they decide on the host which
clips exist (`clip_starts`), as `np.sum(clips[-1][1]) == 0` does in the reference.  The compute stream is never waited for.

Truth may also come as boxes (BoxTruth: per frame a few rects, as UCF101-24 annotates it).  The host then knows which frames hold truth
inside the crop before anything is uploaded, so that wait, the flags launch and the truth upload fall away: the rect table goes up behind the
frames and pc_paint_boxes (csrc/truthboxes.hip) paints the truth part of the video's buffer on the copy stream.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import capi, evalmetrics, ops, spec
from .plan import Plan
from .valstep import PlanEngine

MAX_LAUNCH_CLIPS = 32          # clips of one pc_eval_clips_from_u8 launch


# ---------------------------------------------------------------------- pure host functions (tests/test_evalstep_cpu.py)
def centre_crop(H, W, hw):
    """datasets/ucf_dataloader_eval.py:100-103: (h0, w0) of the hw x hw centre crop, int(margin / 2)."""
    return int((H - hw) / 2), int((W - hw) / 2)


def clip_starts(F, flags, f_skip=2):
    """First frames of the clips evaluate_ucf101.py:79-97 keeps, in its order: i + j for i = 0, 8 * f_skip, ..., j = 0..f_skip-1; frame k of a
    clip is start + k * f_skip; a clip is kept if one of its frames below F has a non-zero flag (flags[f]: truth pixels of frame f)."""
    flags = np.asarray(flags).reshape(-1)
    out = []
    for i in range(0, F, 8 * f_skip):
        for j in range(f_skip):
            if any(flags[f] != 0 for f in range(i + j, min(i + j + 8 * f_skip, F), f_skip)):
                out.append(i + j)
    return out


def ring_place(pos, rows, capacity, bs):
    """Where a video of `rows` clip rows goes in a ring of `capacity` rows whose next free row is `pos`: contiguous, from row 0 if it would
    run over the end.  -> (first row, next free row).  A video may take at most capacity - bs rows."""
    if rows < 1:
        raise ValueError("a video of %d clips takes no rows" % rows)
    if rows > capacity - bs:
        raise ValueError("a video of %d clips needs more than capacity - bs = %d - %d rows of the tables" % (rows, capacity, bs))
    row0 = pos if pos + rows <= capacity else 0
    return row0, row0 + rows


def vote(pred):
    """np.argmax(np.mean(pred, axis=0)) as pc_video_vote computes it: the rows added in order in float32, one division, the first maximum."""
    p = np.asarray(pred, np.float32)
    s = p[0].copy()
    for r in p[1:]:
        s = (s + r).astype(np.float32)
    m = (s / np.float32(p.shape[0])).astype(np.float32)
    best = 0
    for j in range(1, m.size):
        if (np.isnan(m[j]) and not np.isnan(m[best])) or m[j] > m[best]:
            best = j
    return best


def _as_u8(a, what):
    """numpy / host tensor / device tensor -> torch uint8 tensor (no copy), or ValueError."""
    t = a if torch.is_tensor(a) else (torch.from_numpy(a) if isinstance(a, np.ndarray) else None)
    if t is None or t.dtype != torch.uint8:
        raise ValueError("%s: uint8 frames as numpy array or torch tensor, got %s" % (what, getattr(a, "dtype", type(a))))
    return t


def _slice_clip(a, b, n):
    """slice(a, b).indices(n)[:2] on integer arrays, an empty range as (start, start): how numpy clips x[a:b] on an axis of n -- a negative
    bound counts from the end."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    lo = np.where(a < 0, np.maximum(a + n, 0), np.minimum(a, n))
    hi = np.where(b < 0, np.maximum(b + n, 0), np.minimum(b, n))
    return lo, np.maximum(hi, lo)


def pick_annotation(annotations):
    """The annotation the eval loader paints (datasets/ucf_dataloader_eval.py:134-140): the first, or with more than one a draw of
    np.random.randint -- consumed only then, as the loader consumes it.  -> its index."""
    return int(np.random.randint(0, len(annotations))) if len(annotations) > 1 else 0


class BoxTruth:
    """A video's truth as boxes: shape = (F, H, W) and rects, int32 [F, R, 5] -- per frame R rects (x0, x1, y0, y1, value), half-open, inside
    the frame, painted in table order, so that a later rect overwrites an earlier one; a rect with x1 == x0, y1 == y0 or value 0 paints
    nothing (an unused slot is all zeros).  What EvalEngine.add_video and DetectEngine.score / sweep take next to a dense uint8 truth: the
    table goes to the device and pc_paint_boxes paints the map there.  Host only; `dense` is the definition the device is held to."""
    MAX_RECTS, WORDS = 32, 5               # ops.BOX_MAX, ops.BOX_WORDS (PC_BOX_MAX, PC_BOX_WORDS of include/picons.h)

    def __init__(self, shape, rects):
        try:
            F, H, W = (int(v) for v in shape)
        except (TypeError, ValueError):
            raise ValueError("BoxTruth: shape %r is not (F, H, W)" % (shape,)) from None
        if F < 1 or H < 1 or W < 1:
            raise ValueError("BoxTruth: shape %r: F, H, W must be at least 1" % ((F, H, W),))
        r = np.asarray(rects)
        if r.dtype.kind not in "iu" or r.ndim != 3 or r.shape[0] != F or r.shape[2] != self.WORDS:
            raise ValueError("BoxTruth: rects must be an integer array [%d, R, %d], got %s %s" % (F, self.WORDS, r.dtype, r.shape))
        if not 1 <= r.shape[1] <= self.MAX_RECTS:
            raise ValueError("BoxTruth: R = %d rects per frame outside 1..%d" % (r.shape[1], self.MAX_RECTS))
        r = r.astype(np.int64)
        x0, x1, y0, y1, v = (r[..., k] for k in range(5))
        if ((x0 < 0) | (x0 > x1) | (x1 > W)).any():
            raise ValueError("BoxTruth: a rect does not keep 0 <= x0 <= x1 <= W = %d" % W)
        if ((y0 < 0) | (y0 > y1) | (y1 > H)).any():
            raise ValueError("BoxTruth: a rect does not keep 0 <= y0 <= y1 <= H = %d" % H)
        if ((v < 0) | (v > 255)).any():
            raise ValueError("BoxTruth: a rect's value lies outside 0..255")
        self.shape = (F, H, W)
        self.rects = np.ascontiguousarray(r, dtype=np.int32)

    @classmethod
    def from_xywh(cls, boxes, H, W, values=None):
        """boxes: an int array [F, R, 4] of (x, y, w, h) as annotations hold them, clipped exactly as numpy clips bbox[f, y:y+h, x:x+w] -- a
        negative x or y counts from the far edge, a box that is empty after that paints nothing.  values: None (every slot 1) or R values,
        slot r's."""
        b = np.asarray(boxes)
        if b.dtype.kind not in "iu" or b.ndim != 3 or b.shape[2] != 4:
            raise ValueError("BoxTruth.from_xywh: boxes must be an integer array [F, R, 4], got %s %s" % (b.dtype, b.shape))
        F, R = b.shape[:2]
        vals = np.ones(R, np.int64) if values is None else np.asarray(values)
        if vals.shape != (R,) or vals.dtype.kind not in "iu":
            raise ValueError("BoxTruth.from_xywh: values must be %d integers, one per slot" % R)
        b = b.astype(np.int64)
        x0, x1 = _slice_clip(b[..., 0], b[..., 0] + b[..., 2], int(W))
        y0, y1 = _slice_clip(b[..., 1], b[..., 1] + b[..., 3], int(H))
        return cls((F, H, W), np.stack([x0, x1, y0, y1, np.broadcast_to(vals.astype(np.int64), (F, R))], axis=2))

    @classmethod
    def from_annotations(cls, anns, F, H, W, values=None):
        """Annotations (start, end, label, boxes, ...), annotation i in slot i with value i + 1 (values: others), frames start ..
        min(F, end + 1) - 1 each, boxes[f - start] = (x, y, w, h): what painting them in order with their values gives -- the actors of
        DetectEngine.score(actors=A)."""
        anns = list(anns)
        boxes = np.zeros((int(F), max(len(anns), 1), 4), np.int64)
        for i, ann in enumerate(anns):
            start, end = int(ann[0]), int(ann[1])
            if start < 0:
                raise ValueError("BoxTruth: annotation %d starts at frame %d" % (i, start))
            for f in range(start, min(int(F), end + 1)):
                boxes[f, i] = ann[3][f - start]
        return cls.from_xywh(boxes, H, W, np.arange(1, boxes.shape[1] + 1) if values is None else values)

    @classmethod
    def from_annotation(cls, ann, F, H, W, value=1):
        """One annotation as the eval loader's load_video paints it (datasets/ucf_dataloader_eval.py:142-147), with `value`."""
        return cls.from_annotations([ann], F, H, W, [value])

    @property
    def nbytes(self):
        """The bytes of the table: what travels instead of F * H * W."""
        return int(self.rects.nbytes)

    def dense(self, binary=False):
        """numpy uint8 [F, H, W]: the rects painted in table order on the host (binary: 1 for every value that paints)."""
        F, H, W = self.shape
        out = np.zeros(self.shape, np.uint8)
        for f in range(F):
            for x0, x1, y0, y1, v in self.rects[f]:
                if v & 255:
                    out[f, y0:y1, x0:x1] = 1 if binary else v
        return out

    def flags(self, h0, w0, S):
        """int32 [F]: 1 where a rect of the frame that paints meets the S x S crop at (h0, w0), else 0 -- non-zero exactly where
        pc_truth_frame_flags of dense() is: the last rect over a pixel that a painting rect covers is itself one that paints."""
        x0, x1, y0, y1, v = (self.rects[..., k] for k in range(5))
        hit = (v != 0) & (np.maximum(x0, w0) < np.minimum(x1, w0 + S)) & (np.maximum(y0, h0) < np.minimum(y1, h0 + S))
        return hit.any(axis=1).astype(np.int32)


# What a caller hands in next to a video -- EvalEngine.add_video, DetectEngine.score / sweep (who) -- checked on the host: no GPU use.
def check_truth(who, truth, F, H, W, video=None):
    """A truth mask (of video `video` of a pass): uint8, of shape (F, H, W) or (F, H, W, 1) -> torch uint8 [F, H, W] (no copy), or a BoxTruth
    of shape (F, H, W) -> itself; or ValueError."""
    name = "%s: truth" % who if video is None else "%s: truth of video %d" % (who, video)
    if isinstance(truth, BoxTruth):
        if truth.shape != (F, H, W):
            raise ValueError("%s has shape %s, expected (%d, %d, %d) or (%d, %d, %d, 1)" % (name, tuple(truth.shape), F, H, W, F, H, W))
        r = truth.rects                      # a table changed behind the constructor's back: what sizes the upload and the launch is looked at again
        if not (isinstance(r, np.ndarray) and r.dtype == np.int32 and r.ndim == 3 and r.shape[0] == F and r.shape[2] == BoxTruth.WORDS
                and 1 <= r.shape[1] <= BoxTruth.MAX_RECTS and r.flags.c_contiguous):
            raise ValueError("%s: rects must be a contiguous int32 array [%d, R, %d] with R in 1..%d, got %s %s"
                             % (name, F, BoxTruth.WORDS, BoxTruth.MAX_RECTS, getattr(r, "dtype", type(r)), getattr(r, "shape", None)))
        return truth
    t = _as_u8(truth, name)
    if t.dim() == 4 and t.shape[3] == 1:
        t = t.reshape(t.shape[:3])
    if tuple(t.shape) != (F, H, W):
        raise ValueError("%s has shape %s, expected (%d, %d, %d) or (%d, %d, %d, 1)" % (name, tuple(truth.shape), F, H, W, F, H, W))
    return t


def check_label(who, label, C):
    """A class id: an int in [0, C) -> int, or ValueError."""
    try:
        lab = int(label)
    except (TypeError, ValueError):
        raise ValueError("%s: label %r is not a class id" % (who, label)) from None
    if lab != label or not 0 <= lab < C:
        raise ValueError("%s: label %r outside [0, %d)" % (who, label, C))
    return lab


def check_counts(who, truths, labels, n):
    """As many truths and labels as the n picked videos -> (truths, labels) as lists, or ValueError."""
    truths, labels = list(truths), list(labels)
    if not (len(truths) == len(labels) == n):
        raise ValueError("%s: %d truths and %d labels for %d videos" % (who, len(truths), len(labels), n))
    return truths, labels


class ClipEngine(PlanEngine):
    """What the engines that run decoded uint8 video through the eval plan share (EvalEngine here, detect.DetectEngine): one plan of `bs` clips
    whose first conv reads the clip tensor as the clip kernel writes it, the upload pool behind a copy stream, batch forming (pack on / off),
    the ring of class-score rows, and the batch itself (_run_batch) with three steps left to the subclass: _cut (the clip-making launch;
    its last argument is the clip count of the whole segment the launch's clips belong to), _collect (what is read off a video segment's logits)
    and _finish (a video's last clip has run)."""

    def _setup(self, bs, hw, num_classes, device, state, engine, capacity, seed, f_skip, pack, on_batch):
        if not torch.cuda.is_available():
            raise RuntimeError("%s needs a GPU: the hot path is HIP-only (no CPU fallback)" % type(self).__name__)
        if bs < 1 or capacity <= bs:
            raise ValueError("bs must be at least 1 and capacity larger than bs")
        capi.lib()
        lay = self._bind(bs, hw, num_classes, device, state, seed, engine)
        self.capacity, self.f_skip, self.pack, self.on_batch = capacity, f_skip, bool(pack), on_batch
        c = self.c = self._build(bs, lay)
        p = c.plan
        c.ops["fwd"][p.op_to_ndhwc[0]]["i"][1] = 0                      # N = 0, for good: the clip kernel writes the stem's tensor itself
        self._view(c, p.in_cls, bs).fill_(500.0)                        # the reference's empty_action (:121-122) as the module's eval slot leaves it
        self._view(c, p.in_labeled, bs, torch.int32).fill_(500)
        self.img = self._view(c, p.img.ref, bs * self.per * 4)          # [bs][8][hw][hw][4]
        self.img.zero_()                                                # slots no batch has filled yet hold numbers, not whatever the allocator left
        self.out = self._view(c, p.out.ref, bs * self.per)
        self.pred = self._view(c, p.pred, bs * self.C).view(bs, self.C)
        self.scores = torch.zeros(capacity, self.C, device=self.dev)
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.pin = None                      # page-locked staging of one video (frames, then truth); free again when its upload has run
        self.pool = []                       # device buffers of videos: dict(buf, free: event after the last launch that read it, or None if in use)
        self.gen = self.gen_done = 0
        self.m = 0                           # clips of the last batch
        self._reset()

    def _plan(self, n):
        p = Plan(self.C, self.hw, n=n, groups=1, training=False)
        p.build_forward()
        return p

    def _reset(self):
        self.pos = 0                         # next free row of the ring
        self.batch = []                      # segments of the batch being filled: (video record, first clip, count)
        self.fill = 0
        self.live = []                       # videos with clips not yet run, in arrival order
        self.n_videos = self.n_skipped = self.n_clips = 0

    # ------------------------------------------------------------------ the pass
    def begin(self, pack=None):
        """Start a pass (pack: how batches are formed from here on): the subclass's results cleared (_clear), an empty ring, and the weight
        layouts (the `prep` and `prep_late` lists) due again in front of the first batch -- the weights do not change during a pass.  Behind a
        StepEngine, the pass waits for its lanes."""
        for v in self.live:
            self._release(v)
        self._reset()
        if pack is not None:
            self.pack = bool(pack)
        self.gen += 1
        self._clear()
        if self.side:
            ops.streams_fanin(torch.cuda.current_stream(self.dev), self.side)

    def _acquire(self, nbytes):
        """A device buffer of at least nbytes that no launch still to run reads -- the copy stream waits (on the device) for the launches that did."""
        best = None
        for e in self.pool:
            if e["free"] is not None and e["buf"].numel() >= nbytes and (best is None or e["buf"].numel() < best["buf"].numel()):
                best = e
        if best is None:
            main = torch.cuda.current_stream(self.dev)
            for i, e in enumerate(self.pool):
                if e["free"] is not None:                # a free one that is too small makes room for the new one
                    e["buf"].record_stream(main)
                    del self.pool[i]                     # (by position: comparing the entries would compare their tensors)
                    break
            with torch.cuda.stream(self.copy_stream):
                best = dict(buf=torch.empty((nbytes + (1 << 20) - 1) >> 20 << 20, dtype=torch.uint8, device=self.dev), free=None)
            self.pool.append(best)
        else:
            self.copy_stream.wait_event(best["free"])
        best["free"] = None
        return best

    def _release(self, v):
        """The last launch that reads the video has been enqueued on the compute stream: its buffer is free once that launch has run."""
        if v.entry is not None:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.dev))
            v.entry["free"] = ev
            v.entry = None
        v.video = v.truth = None             # a caller's device tensors: stream order on the compute stream keeps them until here

    def _upload(self, v, t=None):
        """-> (video, truth or None, entry) on the device, the upload (if any) enqueued on the copy stream."""
        if v.is_cuda or (t is not None and t.is_cuda):
            if t is None:
                v = v.to(self.dev)
            elif not (v.is_cuda and t.is_cuda):
                v, t = v.to(self.dev), t.to(self.dev)
            self.copy_stream.wait_stream(torch.cuda.current_stream(self.dev))        # whatever produced them
            return v.contiguous(), (None if t is None else t.contiguous()), None
        nv, nt = v.numel(), (0 if t is None else t.numel())
        o_t = (nv + 255) // 256 * 256
        if self.pin is None or self.pin.numel() < o_t + nt:
            self.pin = torch.empty(o_t + nt, dtype=torch.uint8).pin_memory()
        self.pin[:nv].view(v.shape).copy_(v)
        if t is not None:
            self.pin[o_t:o_t + nt].view(t.shape).copy_(t)
        e = self._acquire(o_t + nt)
        with torch.cuda.stream(self.copy_stream):
            e["buf"][:o_t + nt].copy_(self.pin[:o_t + nt], non_blocking=True)
        return e["buf"][:nv].view(v.shape), (None if t is None else e["buf"][o_t:o_t + nt].view(t.shape)), e

    def _width(self, rec):
        """Slots of the batch, and rows of the ring, a clip of this video takes: 1, but for the views of detect.DetectEngine."""
        return 1

    def _join(self, rec, row0, pos):
        """A video with rec.rows ring rows (its clips times _width) takes the rows ring_place gave it, and its clips join the batches.  A clip's
        _width slots always share a batch: a segment (video, first clip, clips) takes clips * _width consecutive slots."""
        if any(row0 < o.row0 + o.rows and o.row0 < row0 + rec.rows for o in self.live):
            self.flush()                     # rows of a video whose clips still wait for a full batch: run them first (pack=True, a small ring)
        rec.row0, self.pos = row0, pos
        self.live.append(rec)
        self.n_videos += 1
        clips, w = len(rec.starts), self._width(rec)
        self.n_clips += clips
        if self.pack:
            first = 0
            while first < clips:
                take = min(clips - first, (self.bs - self.fill) // w)
                if take == 0:                # (w > 1 only) not one more clip fits: the batch runs short
                    self._run_batch()
                    continue
                self.batch.append((rec, first, take))
                self.fill += take * w
                first += take
                if self.fill == self.bs:
                    self._run_batch()
        else:
            for i in range(0, clips, self.bs // w):
                self.batch.append((rec, i, min(self.bs // w, clips - i)))
                self._run_batch()

    def flush(self):
        """Run the clips that wait for a full batch (pack=True) as a short one."""
        self._run_batch()

    def _run_batch(self):
        if not self.batch:
            return
        c = self.c
        main = torch.cuda.current_stream(self.dev)
        slot = 0
        for rec, first, n in self.batch:                                       # one clip-making launch per video segment (32 clips at most each)
            if not rec.waited:
                main.wait_event(rec.ready)
                rec.waited = True
            for q in range(0, n, MAX_LAUNCH_CLIPS):
                self._cut(rec, first + q, min(MAX_LAUNCH_CLIPS, n - q), slot + q, n)
            if first + n == len(rec.starts):
                self._release(rec)
            slot += n * self._width(rec)
        self.m = slot
        if self.gen_done != self.gen:                                          # first batch of the pass: the weight layouts
            ops.run_ops(c.ops["prep"])
            ops.run_ops(c.ops["prep_late"])
            self.gen_done = self.gen
        ops.run_ops(c.ops["fwd"])
        slot = 0
        for rec, first, n in self.batch:
            self._collect(rec, first, n, slot)
            w = self._width(rec)
            r = rec.row0 + first * w
            if w == 1:
                self.scores[r:r + n].copy_(self.pred[slot:slot + n])
            else:                                                              # slots view-major, rows clip-major: row0 + clip * w + view
                self.scores[r:r + n * w].view(n, w, self.C).copy_(self.pred[slot:slot + n * w].view(w, n, self.C).transpose(0, 1))
            slot += n * w
        if self.on_batch is not None:
            self.on_batch(self.m, *self.outputs())
        for rec, first, n in self.batch:
            rec.done += n
            if rec.done == len(rec.starts):                                    # the video's last clip has run
                self._finish(rec)
                self.live = [o for o in self.live if o is not rec]
        self.batch, self.fill = [], 0

    def outputs(self):
        """(output (m,1,8,H,W) logits, predicted_action (m,C)) of the last batch's m slots: views of the plan's arena."""
        return self.out[:self.m * self.per].view(self.m, 1, spec.FRAMES, self.hw, self.hw), self.pred[:self.m]


class EvalEngine(ClipEngine):
    """Evaluates the weights in the flat buffers P, R: a StepEngine's own (StepEngine.eval_engine: no copy, behind its lanes) or, built from a
    state dict, buffers of its own (load_state per checkpoint).

    begin() once per pass, add_video(frames_u8, truth_u8, label) per video, results() at the end -- or evaluate(videos).  pack=False: batches
    of up to `bs` clips of ONE video, as the reference forms them; pack=True: clips of consecutive videos share full batches.  A batch of
    m < bs clips runs on the same plan: in eval mode a clip's outputs do not depend on its neighbours, the stale slots cost time only."""

    def __init__(self, bs=14, hw=224, num_classes=24, device="cuda:0", state=None, engine=None, capacity=256, seed=47, f_skip=2, pack=False, on_batch=None):
        self._setup(bs, hw, num_classes, device, state, engine, capacity, seed, f_skip, pack, on_batch)
        self.gt = torch.zeros(bs * self.per, device=self.dev)           # [bs][8][hw][hw], the truth of the batch in flight
        self.counts = torch.zeros(capacity * spec.FRAMES, 3, dtype=torch.int32, device=self.dev)
        # the accumulators of evaluate_ucf101.py:66-72 in ONE int32 buffer, so that a pass ends with one device-to-host copy
        C_, T = self.C, evalmetrics.N_THR
        self.tables = torch.zeros(2 * C_ * T + 2 * C_ + 1, dtype=torch.int32, device=self.dev)
        self.acc = self._accumulator(self.tables)
        self.pin_flags = self.dev_flags = None
        # a BoxTruth video has no host wait of its own, so the one staging buffer above would be filled again while the upload in front still
        # reads it: two page-locked slots with their upload events, as DetectEngine.add_video has them
        self.up_pin, self.up_done, self.up_slot = [None, None], [None, None], 0

    def _accumulator(self, flat):
        C_, T = self.C, evalmetrics.N_THR
        a = evalmetrics.MapAccumulator.__new__(evalmetrics.MapAccumulator)
        a.n_classes = C_
        a.frame_hits, a.video_hits = flat[:C_ * T].view(C_, T), flat[C_ * T:2 * C_ * T].view(C_, T)
        a.n_frames, a.n_vids, a.n_correct = flat[2 * C_ * T:2 * C_ * T + C_], flat[2 * C_ * T + C_:2 * C_ * T + 2 * C_], flat[2 * C_ * T + 2 * C_:]
        return a

    def _clear(self):
        self.tables.zero_()

    def _cut(self, rec, first, k, slot, seg):
        per = self.per
        ops.eval_clips_from_u8(rec.video, rec.truth, rec.h0, rec.w0, self.hw, rec.starts[first:first + k], self.f_skip,
                               out=(self.img[slot * per * 4:(slot + k) * per * 4], self.gt[slot * per:(slot + k) * per]))

    def _collect(self, rec, first, n, slot):
        T, per = spec.FRAMES, self.per
        capi.call("pc_seg_frame_counts", ops.ptr(self.out[slot * per:]), ops.ptr(self.gt[slot * per:]), T * n, self.hw * self.hw,
                  ops.ptr(self.counts[(rec.row0 + first) * T:]), ops.stream())

    def _finish(self, rec):
        """The video's rows into the tables."""
        a, T = self.acc, spec.FRAMES
        ops.map_accumulate(self.counts[rec.row0 * T:(rec.row0 + rec.rows) * T], rec.label, a.frame_hits, a.video_hits, a.n_frames, a.n_vids)
        ops.video_vote(self.scores[rec.row0:rec.row0 + rec.rows], rec.label, a.n_correct)

    def check_video(self, frames, truth, label):
        """Refuse (ValueError) a video the engine cannot take, before anything is enqueued or changed.  -> (frames, truth [F,H,W], label)."""
        v = _as_u8(frames, "frames")
        if v.dim() != 4 or v.shape[3] != 3 or v.shape[0] < 1:
            raise ValueError("frames: shape %s, expected (F, H, W, 3)" % (tuple(v.shape),))
        F, H, W = (int(s) for s in v.shape[:3])
        if H < self.hw or W < self.hw:
            raise ValueError("frames of %d x %d are smaller than the %d x %d crop" % (H, W, self.hw, self.hw))
        return v, check_truth("add_video", truth, F, H, W), check_label("add_video", label, self.C)

    def add_video(self, frames_u8, truth_u8, label):
        """One video: frames [F,H,W,3] uint8, truth [F,H,W] or [F,H,W,1] uint8 (numpy, host tensor or device tensor), class id.  Uploaded through
        page-locked memory on the copy stream; its kept clips join the batches.  -> the number of clips (0: "Video has no bounding boxes",
        evaluate_ucf101.py:99-101, the video is skipped)."""
        v, t, lab = self.check_video(frames_u8, truth_u8, label)
        if isinstance(t, BoxTruth):
            return self._add_video_boxes(v, t, lab)
        F, H, W = (int(s) for s in v.shape[:3])
        h0, w0 = centre_crop(H, W, self.hw)
        if self.dev_flags is None or self.dev_flags.numel() < F:
            with torch.cuda.stream(self.copy_stream):                # allocated where it is used: every frame's flag is a plain store, no fill
                self.dev_flags = torch.empty(max(F, 256), dtype=torch.int32, device=self.dev)
            self.pin_flags = torch.zeros(max(F, 256), dtype=torch.int32).pin_memory()
        dv, dt, entry = self._upload(v, t)
        rec = SimpleNamespace(video=dv, truth=dt, entry=entry, F=F, H=H, W=W, h0=h0, w0=w0, label=lab, ready=torch.cuda.Event(), waited=False)
        with torch.cuda.stream(self.copy_stream):
            ops.truth_frame_flags(dt, h0, w0, self.hw, self.dev_flags)
            self.pin_flags[:F].copy_(self.dev_flags[:F], non_blocking=True)
            rec.ready.record(self.copy_stream)
        rec.ready.synchronize()              # the one host wait of the video: F integers, on the copy stream
        rec.starts = clip_starts(F, self.pin_flags[:F].numpy(), self.f_skip)
        rec.rows, rec.done = len(rec.starts), 0
        if not rec.starts:
            self._release(rec)
            self.n_skipped += 1
            return 0
        try:
            row0, pos = ring_place(self.pos, rec.rows, self.capacity, self.bs)
        except ValueError:
            self._release(rec)
            raise
        self._join(rec, row0, pos)
        return rec.rows

    def _add_video_boxes(self, v, bt, lab):
        """add_video with the truth as a BoxTruth.  Which frames hold truth inside the crop is known on the host (BoxTruth.flags), so the
        clips are decided before anything is enqueued: a video without one costs nothing, and for the others the frames go up alone, the
        rect table behind them through the same page-locked slot, and pc_paint_boxes writes the truth part of the pool entry on the copy
        stream in front of rec.ready -- binary, whatever the values: pc_seg_frame_counts needs the truth value 1.  No flags launch and no
        wait per video: the host waits at most for its own upload of two videos ago, if that has not left its slot yet."""
        F, H, W = bt.shape
        h0, w0 = centre_crop(H, W, self.hw)
        starts = clip_starts(F, bt.flags(h0, w0, self.hw), self.f_skip)
        if not starts:
            self.n_skipped += 1
            return 0
        row0, pos = ring_place(self.pos, len(starts), self.capacity, self.bs)
        slot = self.up_slot
        self.up_slot ^= 1
        if self.up_done[slot] is not None and not self.up_done[slot].query():
            self.up_done[slot].synchronize()                          # an upload on the copy stream, two videos back: never the compute stream
        host = not v.is_cuda
        nv, nt, nr = v.numel(), F * H * W, bt.nbytes
        o_t = (nv + 255) // 256 * 256 if host else 0                  # where the truth starts in the pool entry, and the table in the slot
        pin = self.up_pin[slot]
        if pin is None or pin.numel() < o_t + nr:
            pin = self.up_pin[slot] = torch.empty(o_t + nr, dtype=torch.uint8).pin_memory()
        if host:
            pin[:nv].view(v.shape).copy_(v)
        table = pin[o_t:o_t + nr].view(torch.int32).view(bt.rects.shape)
        table.copy_(torch.from_numpy(bt.rects))
        main = torch.cuda.current_stream(self.dev)
        if host:
            entry = self._acquire(o_t + nt)                           # sized for frames + truth, as with a dense truth; the truth part is painted
        else:
            entry, dv = None, v.to(self.dev).contiguous()
            self.copy_stream.wait_stream(main)                        # whatever produced the frames
        rec = SimpleNamespace(entry=entry, F=F, H=H, W=W, h0=h0, w0=w0, label=lab, ready=torch.cuda.Event(), waited=False, starts=starts,
                              rows=len(starts), done=0)
        with torch.cuda.stream(self.copy_stream):
            if host:
                entry["buf"][:nv].copy_(pin[:nv], non_blocking=True)
                dv, dt = entry["buf"][:nv].view(v.shape), entry["buf"][o_t:o_t + nt].view(F, H, W)
            else:
                dt = torch.empty(F, H, W, dtype=torch.uint8, device=self.dev)
                dt.record_stream(main)                                # made on the copy stream, read and let go on the compute stream
            rects = torch.empty(bt.rects.shape, dtype=torch.int32, device=self.dev)
            rects.copy_(table, non_blocking=True)
            ops.paint_boxes(rects, F, H, W, binary=True, truth=dt)
            rec.ready.record(self.copy_stream)
        self.up_done[slot] = rec.ready
        rec.video, rec.truth = dv, dt
        self._join(rec, row0, pos)
        return rec.rows

    def results(self):
        """The pass's one device-to-host copy -> the dict of evalmetrics.MapAccumulator.result()."""
        self.flush()
        return self._accumulator(self.tables.cpu()).result()

    def evaluate(self, videos, pack=False):
        """One pass over an iterable of (frames_u8, truth_u8, label) -> results()."""
        self.begin(pack)
        for frames, truth, label in videos:
            self.add_video(frames, truth, label)
        return self.results()
