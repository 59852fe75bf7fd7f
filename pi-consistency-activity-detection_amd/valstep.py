"""The validation pass on one MI355X: the reference's val_model_interface + validate (main_ucf101.py:33-47, 226-278) with the eval
forward replayed from an op plan and every loss, the per-clip IoU sums and the accuracy count computed by pc_val_metrics
(csrc/valmetrics.hip) behind it.  Nothing comes back to the host per batch: each batch leaves one small record in a device table,
read with one D2H at the end of the pass (`results`), and `summarize` turns the records into the numbers validate prints and returns.

The eval plan is replayed on ONE stream (torch's current one).  The lane tags of plan.py are laid out for the training step (weight
gradient lane, skip-conv lane, late weight prep joined in front of Mixed_3b); an eval forward has none of that work to spread, and the
nn.Module's eval slot -- the path this engine is checked against -- is a single-lane plan too.
"""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from . import capi, ops, spec, synthetic
from .plan import Plan

KEYS = ("data", "action", "loc_msk")


class PlanEngine:
    """What the engines that replay an eval plan share (ValEngine here, evalstep.EvalEngine): the flat parameter / running-statistics buffers
    P, R -- a StepEngine's own (no copy) or, built from a state dict, buffers of their own -- a plan resolved over an arena, and views into it.
    A subclass provides _plan(n)."""

    def _bind(self, bs, hw, num_classes, device, state, seed, engine):
        """Device, sizes, P / R and the lanes to fan in; -> the primary plan (not yet resolved)."""
        self.engine = engine
        if engine is not None:
            self.dev, self.hw, self.C = engine.dev, engine.hw, engine.C
            self.P, self.R = engine.P, engine.R
            self.side = list(engine.side) + ([engine.main] if engine.main is not None else [])
        else:
            self.dev, self.hw, self.C = torch.device(device), hw, num_classes
            self.side = []
        torch.cuda.set_device(self.dev)
        self.bs = bs
        self.per = spec.FRAMES * self.hw * self.hw                 # pixels of one clip's mask
        lay = self._plan(bs)
        self.pshape, self.poff, self.roff = lay.pshape, lay.poff, lay.roff
        if engine is None:
            self.P = torch.zeros(lay.nparams, device=self.dev)
            self.R = torch.zeros(lay.nrunning, device=self.dev)
            self.load_state(state if state is not None else synthetic.init_state(seed, num_classes))
        elif (lay.nparams, lay.nrunning, lay.poff, lay.roff) != (engine.plan.nparams, engine.plan.nrunning, engine.plan.poff, engine.plan.roff):
            raise RuntimeError("the eval plan lays out the parameters differently from the engine's plan")
        return lay

    def _build(self, n, p=None):
        p = p or self._plan(n)
        arena = torch.empty(p.arena_bytes + 256, device=self.dev, dtype=torch.uint8)
        base = (arena.data_ptr() + 255) // 256 * 256
        c = SimpleNamespace(plan=p, n=n, arena=arena, a0=base - arena.data_ptr(), gen=-1)
        c.ops = p.resolve(dict(A=base, P=self.P.data_ptr(), G=0, M=0, V=0, R=self.R.data_ptr()))
        if len(p.op_to_ndhwc) != 1:
            raise RuntimeError("an eval plan converts one clip tensor, this one %d" % len(p.op_to_ndhwc))
        view = lambda ref, nf, dt=torch.float32: self._view(c, ref, nf, dt)
        p.upload_consts(view)
        return c

    @staticmethod
    def _view(c, ref, nfloats, dtype=torch.float32):
        o = c.a0 + ref[1]
        return c.arena[o:o + 4 * nfloats].view(dtype)

    def load_state(self, state):
        """Reference-layout state_dict (numpy or torch values) into the engine's OWN buffers."""
        if self.engine is not None:
            raise RuntimeError("this %s reads its StepEngine's buffers: load the state there" % type(self).__name__)
        T = lambda v: (v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(self.dev, torch.float32)
        for k, shp in self.pshape.items():
            o = self.poff[k]
            self.P[o:o + int(np.prod(shp))].copy_(T(state[k]).reshape(-1))
        for k, o in self.roff.items():
            v = T(state[k])
            self.R[o:o + v.numel()].copy_(v)


class ValEngine(PlanEngine):
    """Validates the weights in the flat parameter / running-statistics buffers P, R: a StepEngine's own (StepEngine.val_engine: no copy,
    validation sees what the last train step left) or, built from a state dict, buffers of its own.

    begin() once per pass, val_step(minibatch) per batch (never synchronises), results() at the end.  `bs` sizes the primary plan; a
    shorter (last) batch runs on a plan for its own size, built on first use, with an arena of its own (at most SHORT_PLANS are kept)."""

    SHORT_PLANS = 2

    def __init__(self, bs, hw=224, num_classes=24, device="cuda:0", state=None, seed=47, capacity=64, engine=None):
        if not torch.cuda.is_available():
            raise RuntimeError("ValEngine needs a GPU: the hot path is HIP-only (no CPU fallback)")
        if bs < 1 or capacity < 1:
            raise ValueError("bs and capacity must be at least 1")
        capi.lib()
        lay = self._bind(bs, hw, num_classes, device, state, seed, engine)
        self.capacity = capacity
        self.words = ops.val_record_words(bs)
        self.table = torch.zeros(capacity, self.words, dtype=torch.int32, device=self.dev)
        self.k = 0                       # filled rows of the table
        self._flushed = []               # records read back because the table ran full
        self.gen = 0                     # validation pass; a plan's weight layouts are made once per pass (begin)
        self._primary = self._cur = self._build(bs, lay)
        self._short = OrderedDict()
        # staging: two slots, so that the host fills one while the GPU reads the other
        self.copy_stream = torch.cuda.Stream(device=self.dev)
        self.ready = [torch.cuda.Event(), torch.cuda.Event()]
        self.consumed = [torch.cuda.Event(), torch.cuda.Event()]
        self.used = [False, False]
        self.pin = [{}, {}]              # (key, dtype) -> page-locked tensor
        self.stg = [{}, {}]              # (key, dtype) -> its device copy
        self.hold = [None, None]         # device inputs read in place: kept alive until the slot comes round again
        self.pin_small = [torch.zeros(2 * bs, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.dev_small = [torch.zeros(2 * bs, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self.slot = 0
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=8)        # the gather into page-locked memory, one clip per job (tensor.copy_ releases the GIL)

    # ------------------------------------------------------------------ plans
    def _plan(self, n):
        p = Plan(self.C, self.hw, n=n, groups=1, training=False)
        p.build_forward()
        # behind the forward, in the same list: the batch's truth, class ids and the metrics launch
        p.in_seg = p.alloc(n * self.per)
        p.in_action = p.alloc(n)
        ws = p.alloc(max(ops.val_metrics_ws_floats(n, self.per), 4))
        p.op_metrics = len(p.lists["fwd"])
        p.emit(capi.OP_VAL_METRICS, i=[n, self.C], l=[self.per], p=[p.out.ref, p.in_seg, p.pred, p.in_action, None, ws], lst="fwd", lane=0)
        return p

    def _build(self, n, p=None):
        c = super()._build(n, p)
        self._view(c, c.plan.in_labeled, n, torch.int32).zero_()           # val_model_interface's empty_vector
        return c

    def _activate(self, m):
        if m == self.bs:
            c = self._primary
        else:
            c = self._short.get(m)
            if c is None:
                while len(self._short) >= self.SHORT_PLANS:
                    torch.cuda.current_stream(self.dev).synchronize()       # the evicted arena may still be read by a batch in flight
                    self._short.popitem(last=False)
                c = self._short[m] = self._build(m)
            else:
                self._short.move_to_end(m)
        self._cur = c
        return c

    # ------------------------------------------------------------------ the pass
    def begin(self):
        """Start a validation pass: forget the records of the last one, and have every plan make its weight layouts (the `prep` and
        `prep_late` lists: re-layouts, Winograd transforms, spectral planes) once, in front of its first batch -- the weights do not change
        during the pass.  Both lists read parameters only; what the forward derives from the running statistics stays in the forward list."""
        self.gen += 1
        self.k = 0
        self._flushed = []
        if self.side:            # the last train step's side lanes (weight gradients, the early Adam) write what this pass reads
            ops.streams_fanin(torch.cuda.current_stream(self.dev), self.side)

    def check_minibatch(self, mb):
        """Refuse (ValueError) a minibatch the engine cannot run, before anything is enqueued or changed.  -> (m, action as int64 host array)."""
        try:
            data, action, msk = (mb[k] for k in KEYS)
        except (KeyError, TypeError) as e:
            raise ValueError("validation minibatch needs the keys %s: %r" % (KEYS, e)) from None
        shp = lambda a: tuple(a.shape) if hasattr(a, "shape") else np.shape(a)
        ds = shp(data)
        if len(ds) != 5 or ds[1:] != (3, spec.FRAMES, self.hw, self.hw):
            raise ValueError("data: shape %s, expected (m, 3, %d, %d, %d)" % (ds, spec.FRAMES, self.hw, self.hw))
        m = ds[0]
        if not 1 <= m <= self.bs:
            raise ValueError("minibatch of %d clips on a validation engine built for 1..%d" % (m, self.bs))
        ms = shp(msk)
        if len(ms) < 1 or ms[0] != m or int(np.prod(ms[1:])) != self.per:
            raise ValueError("loc_msk: shape %s, expected (%d, 1, %d, %d, %d)" % (ms, m, spec.FRAMES, self.hw, self.hw))
        act = (action.detach().cpu().numpy() if torch.is_tensor(action) else np.asarray(action)).reshape(-1)
        if act.size != m:
            raise ValueError("action: %d entries for %d clips" % (act.size, m))
        ai = act.astype(np.int64)
        if not np.array_equal(ai, act) or ai.min() < 0 or ai.max() >= self.C:
            raise ValueError("action: class ids must be integers in [0, %d), got %s" % (self.C, act.tolist()))
        return m, ai

    def _stage_big(self, slot, key, t, m):
        """Host tensor -> this slot's device staging in the tensor's own float type (cast on the device); device tensor -> itself."""
        t = t if torch.is_tensor(t) else torch.from_numpy(np.asarray(t))
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float32)
        if t.is_cuda:
            return t.to(self.dev).contiguous()
        k = (key, t.dtype)
        if k not in self.pin[slot]:
            shape = (self.bs,) + tuple(t.shape[1:])
            self.pin[slot][k] = torch.empty(shape, dtype=t.dtype).pin_memory()
            self.stg[slot][k] = torch.empty(shape, dtype=t.dtype, device=self.dev)
        pin, stg = self.pin[slot][k], self.stg[slot][k]
        for f in [self.pool.submit(pin[j].copy_, t[j]) for j in range(m)]:
            f.result()
        with torch.cuda.stream(self.copy_stream):
            stg[:m].copy_(pin[:m], non_blocking=True)
        return stg[:m]

    def val_step(self, minibatch):
        """One validation batch: checked, staged through page-locked memory, forward + metrics enqueued; its record lands in the next row
        of the device table.  Does not synchronise (a full table is read back first; a staging slot waits for the batch that used it two
        calls ago)."""
        m, ai = self.check_minibatch(minibatch)
        if self.k == self.capacity:
            self._flushed += self._fetch()
        c = self._activate(m)
        p, fwd = c.plan, c.ops["fwd"]
        main = torch.cuda.current_stream(self.dev)
        slot = self.slot
        self.slot ^= 1
        if self.used[slot]:
            self.ready[slot].synchronize()                  # the slot's upload of two batches ago: the page-locked side is free again
            self.copy_stream.wait_event(self.consumed[slot])   # and its device side has been read (waited for on the device)
        data = self._stage_big(slot, "data", minibatch["data"], m)
        msk = self._stage_big(slot, "loc_msk", minibatch["loc_msk"], m)
        ps = self.pin_small[slot]
        ps[:m].view(torch.float32).copy_(torch.from_numpy(ai.astype(np.float32)))
        ps[self.bs:self.bs + m].copy_(torch.from_numpy(ai.astype(np.int32)))
        with torch.cuda.stream(self.copy_stream):
            self.dev_small[slot].copy_(ps, non_blocking=True)
            self.ready[slot].record(self.copy_stream)
        self.used[slot] = True
        self.hold[slot] = (data, msk)
        main.wait_event(self.ready[slot])
        if c.gen != self.gen:                               # first batch of the pass on this plan: its weight layouts
            ops.run_ops(c.ops["prep"])
            ops.run_ops(c.ops["prep_late"])
            c.gen = self.gen
        ds = self.dev_small[slot]
        self._view(c, p.in_cls, m).copy_(ds[:m].view(torch.float32))
        self._view(c, p.in_action, m, torch.int32).copy_(ds[self.bs:self.bs + m])
        self._view(c, p.in_seg, m * self.per).copy_(msk.reshape(-1))          # (f64 -> f32 on the device)
        k0 = p.op_to_ndhwc[0]
        fwd[k0]["i"][0] = int(data.dtype == torch.float64)                     # the layout conversion reads the staging as it is
        fwd[k0]["p"][0] = data.data_ptr()
        fwd[p.op_metrics]["p"][4] = self.table[self.k].data_ptr()
        ops.run_ops(fwd)
        self.consumed[slot].record(main)
        self.k += 1

    def _fetch(self):
        rows = self.table[:self.k].cpu().numpy()            # the pass's one device-to-host copy (per `capacity` batches)
        self.k = 0
        return [ops.decode_val_record(r) for r in rows]

    def results(self):
        """The records of every batch since begin(), in order (ops.decode_val_record dicts)."""
        out = self._flushed + self._fetch()
        self._flushed = []
        return out

    def outputs(self):
        """(output (m,1,8,H,W) logits, predicted_action (m,C)) of the last batch: views of its plan's arena."""
        c = self._cur
        return (self._view(c, c.plan.out.ref, c.n * self.per).view(c.n, 1, spec.FRAMES, self.hw, self.hw),
                self._view(c, c.plan.pred, c.n * self.C).view(c.n, self.C))


def summarize(records, epoch=0):
    """What validate (main_ucf101.py:271-278) makes of a pass, from its per-batch records -- no GPU needed.  Losses and accuracy are means
    over BATCHES (np.array(total_loss).mean()), the IoU a mean over the clips with truth; inter / union is divided as Python floats on the
    exact integer counts.  `line` is the line validate prints, `total` what it returns."""
    if not records:
        raise ValueError("summarize: no records")
    tot = float(np.array([r["total"] for r in records]).mean())
    loc = float(np.array([r["loc"] for r in records]).mean())
    cls = float(np.array([r["cls"] for r in records]).mean())
    acc = float(np.array([r["n_correct"] / float(r["B"]) for r in records]).mean())
    total_iou, valid = 0, 0
    for r in records:
        for inter, union, gt in np.asarray(r["counts"]).reshape(-1, 3).tolist():
            if gt > 0:
                total_iou += float(inter) / float(union)
                valid += 1
    avg = total_iou / max(valid, 1)
    line = f'[VAL] epoch-{epoch}, loss-{tot:.3f}, acc-{acc:.3f} [IOU ] {avg:.3f}'
    return dict(total=tot, loc=loc, cls=cls, accuracy=acc, total_IOU=float(total_iou), validiou=valid, average_IOU=float(avg), line=line)
