#!/usr/bin/env python3
"""Validation pass on one MI355X: clips/s of the drop-in's validate() through valstep.ValEngine (forward, losses, IoU sums and accuracy on
the device, one read-back per pass) against validate() with engine=None -- the nn.Module path with torch losses, two .item() syncs, a D2H
of the logits and numpy IoU per batch, whose function body is unchanged from commit 535973b (the parent of the commit that added the
engine).  Both paths consume the same list of synthetic float64 HOST minibatches (the reference's DataLoader contract), so the upload is
inside both timings; each timing is a host clock around a pass that ends with the GPU drained.  The passes alternate between the two
paths; the medians are reported.  Also: pc_val_metrics alone on one batch, as a share of the HBM roof (8 bytes per pixel, read once).

    python tools/bench_val.py [--bs 16] [--hw 224] [--batches 8] [--passes 5] [--warmup 1] [--out profiles/val_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pi-consistency-activity-detection_amd", "dropin"))
import picons_amd  # noqa: F401,E402
from picons_amd import model as pmodel, ops, synthetic, valstep  # noqa: E402

BASELINE_COMMIT = "535973b"
HBM_PEAK_GBS = 8000.0              # spec; a float4 copy reaches about 6300 GB/s on this part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--hw", type=int, default=224)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_val.py measures on a GPU; there is none here")
    if a.passes < 5 or a.batches < 8:
        raise SystemExit("at least five passes of at least eight batches")
    import main_ucf101 as M
    state = synthetic.init_state(47, 24)
    net = pmodel.CapsNet(pt_path=None, hw=a.hw, init="conditioned").cuda()
    net.load_state_dict(state)
    M.model = net
    M.criterion_cls = M.SpreadLoss(num_class=24, m_min=0.2, m_max=0.9)
    M.criterion_seg_1 = torch.nn.BCEWithLogitsLoss()
    M.criterion_seg_2 = M.DiceLoss()
    ve = valstep.ValEngine(a.bs, hw=a.hw, state=state)
    loader = [{k: torch.from_numpy(v) for k, v in synthetic.make_minibatch(a.bs, True, 900 + i, 24, a.hw).items() if k in valstep.KEYS}
              for i in range(a.batches)]

    def one_pass(engine):
        buf = io.StringIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            loss = M.validate(net, loader, 1, engine)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, loss, buf.getvalue().strip().splitlines()[-1]
    for _ in range(max(a.warmup, 1)):
        one_pass(None); one_pass(ve)
    times = {"baseline": [], "engine": []}
    last = {}
    for _ in range(a.passes):
        for name, eng in (("baseline", None), ("engine", ve)):
            dt, loss, line = one_pass(eng)
            times[name].append(dt)
            last[name] = (loss, line)
    clips = a.bs * a.batches
    rate = {k: clips / statistics.median(v) for k, v in times.items()}
    # the metrics kernel alone
    x = torch.randn(a.bs, 1, 8, a.hw, a.hw, device="cuda") * 4
    y = (torch.rand(a.bs, 1, 8, a.hw, a.hw, device="cuda") < 0.2).float()
    p = torch.rand(a.bs, 24, device="cuda")
    act = torch.randint(0, 24, (a.bs,), device="cuda", dtype=torch.int32)
    rec = torch.empty(ops.val_record_words(a.bs), dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.val_metrics_ws_floats(a.bs, 8 * a.hw * a.hw), device="cuda")
    for _ in range(5):
        ops.val_metrics(x, y, p, act, rec, ws)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        ops.val_metrics(x, y, p, act, rec, ws)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 50
    gb = 2 * x.numel() * 4 / 1e9
    out = {"metric": "validation clips/sec (bs=%d clips, 8x%dx%d, float64 host minibatches, %d batches per pass, median of %d passes)" % (a.bs, a.hw, a.hw, a.batches, a.passes),
           "engine": {"value": rate["engine"], "unit": "clips/s", "pass_s": sorted(times["engine"]), "val_loss": last["engine"][0], "line": last["engine"][1]},
           "baseline": {"value": rate["baseline"], "unit": "clips/s", "pass_s": sorted(times["baseline"]), "val_loss": last["baseline"][0], "line": last["baseline"][1],
                        "what": "validate(model, loader, epoch) with engine=None: the function body of commit %s, unchanged" % BASELINE_COMMIT},
           "ratio": rate["engine"] / rate["baseline"], "val_loss_difference": abs(last["engine"][0] - last["baseline"][0]),
           "val_metrics_kernel": {"ms_per_batch": ms, "bound": "hbm", "achieved": gb / (ms * 1e-3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": gb / (ms * 1e-3) / HBM_PEAK_GBS, "algorithmic_bytes": gb * 1e9, "launches": 2}}
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
