#!/usr/bin/env python3
"""AUTHORING CONTAINER ONLY: run the reference's own val_model_interface and validate (/root/reference/main_ucf101.py:33-47, 226-278)
on the batches of tests/valfixture.py with `ValNet` standing in for the network, and record what they compute in
tests/golden/val_epoch.npz: the inputs the losses see (logits, class scores, truth, actions), the per-batch losses and accuracy,
total_IOU, validiou, the return value and the printed line.  The data loader and the model are stubs; the losses, get_accuracy, IOU2
and every line of the two functions are the reference's, executed as is."""
import contextlib
import io
import os
import runpy
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import ref_import  # noqa: E402
from tests import valfixture  # noqa: E402

EPOCH = 7


def main():
    ref_import.install_shims()
    ref_import._stub("datasets.ucf_dataloader", UCF101DataLoader=object)
    ref_import._stub("models.capsules_ucf101", CapsNet=valfixture.ValNet)
    ref = runpy.run_path(os.path.join(ref_import.REF, "main_ucf101.py"), run_name="reference_main")
    validate = ref["validate"]
    G = validate.__globals__
    net = valfixture.ValNet()
    G["model"] = net
    G["criterion_cls"] = ref["SpreadLoss"](num_class=valfixture.NCLS, m_min=0.2, m_max=0.9)
    G["criterion_seg_1"] = torch.nn.BCEWithLogitsLoss(size_average=True)
    G["criterion_seg_2"] = ref["DiceLoss"]()
    batches = [{k: torch.from_numpy(v) for k, v in mb.items()} for mb in valfixture.batches()]
    grabbed, seen = {}, {"logits": [], "scores": []}
    inner = G["val_model_interface"]

    def spy(minibatch):                                  # the reference's function, its outputs noted on the way through
        res = inner(minibatch)
        seen["logits"].append(res[0].detach().numpy().copy())
        seen["scores"].append(res[1].detach().numpy().copy())
        return res
    G["val_model_interface"] = spy

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "validate":
            grabbed.update({k: frame.f_locals[k] for k in ("total_loss", "loc_loss", "class_loss", "accuracy", "total_IOU", "validiou")})
            grabbed["ret"] = arg
    buf = io.StringIO()
    sys.setprofile(prof)
    try:
        with contextlib.redirect_stdout(buf):
            validate(net, batches, EPOCH)
    finally:
        sys.setprofile(None)
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("[VAL]")][0]
    pred = np.concatenate(seen["scores"])
    top2 = np.sort(pred, axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0]).min() > 1e-4, "the fixture must have no arg-max ties"
    out = dict(logits=np.concatenate(seen["logits"]).astype(np.float32), scores=pred.astype(np.float32),
               truth=np.concatenate([mb["loc_msk"] for mb in valfixture.batches()]).astype(np.uint8),
               action=np.concatenate([mb["action"].reshape(-1) for mb in valfixture.batches()]).astype(np.int32),
               sizes=np.asarray(valfixture.SIZES, np.int32), epoch=np.asarray(EPOCH),
               total_loss=np.asarray(grabbed["total_loss"], np.float64), loc_loss=np.asarray(grabbed["loc_loss"], np.float64),
               class_loss=np.asarray(grabbed["class_loss"], np.float64), accuracy=np.asarray(grabbed["accuracy"], np.float64),
               total_IOU=np.asarray(float(grabbed["total_IOU"]), np.float64), validiou=np.asarray(int(grabbed["validiou"])),
               ret=np.asarray(float(grabbed["ret"]), np.float64), line=np.asarray(line))
    path = os.path.join(ROOT, "tests", "golden", "val_epoch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", line, grabbed["total_loss"], grabbed["accuracy"], grabbed["total_IOU"], grabbed["validiou"])
    lg = out["logits"]
    print("planted: +0.0 %d, -0.0 %d, +80 %d, -80 %d" % (int(((lg == 0) & ~np.signbit(lg)).sum()), int(((lg == 0) & np.signbit(lg)).sum()),
                                                         int((lg == 80).sum()), int((lg == -80).sum())))


if __name__ == "__main__":
    main()
