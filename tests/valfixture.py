"""Build-owned synthetic validation set + stand-in network for the validation-pass tests.

The reference's validation (main_ucf101.py:33-47 val_model_interface, :226-278 validate) takes minibatch dicts, runs the network,
three losses, the accuracy and IOU2 per clip.  Its arithmetic is pinned by running THOSE functions (tools/make_val_golden.py,
authoring container only) on the batches below with `ValNet` standing in for the network, and recording what they compute in
tests/golden/val_epoch.npz.  Everything here is numpy PCG64 / plain torch: no reference code."""
import numpy as np
import torch

HW = 16
T = 8
NCLS = 24
SIZES = (4, 4, 3)


class ValNet(torch.nn.Module):
    """Stand-in with the network's signature (capsules_ucf101.py:413,512).  The logits are read off the clip: channel 0 maps [0, 1] to
    [-80, 80] in float32 (0.5 -> exactly 0.0), channel 1 above 0.75 flips the sign (so 0.0 becomes -0.0); the class scores are a fixed
    projection of per-frame channel means."""

    def __init__(self, ncls=NCLS, seed=5):
        super().__init__()
        g = np.random.default_rng(seed)
        self.register_buffer("proj", torch.from_numpy(g.standard_normal((T * 3, ncls)).astype(np.float32)))

    def forward(self, data, classification=None, concat_labels=None, epoch=0, thresh_ep=0):
        data = data.float()
        seg = data[:, 0:1] * 160.0 - 80.0
        seg = torch.where(data[:, 1:2] > 0.75, -seg, seg)                       # (B,1,8,H,W) logits
        feat = data.mean((3, 4)).permute(0, 2, 1).reshape(data.shape[0], -1)     # (B, 8*3)
        pred = torch.sigmoid(feat @ self.proj.to(feat.device) * 4.0)
        return seg, pred, None


def batches(seed=23, ncls=NCLS):
    """-> list of minibatch dicts (float64 data (n,3,8,HW,HW), loc_msk (n,1,8,HW,HW), action (n,1) float32), n = 4, 4, 3.
    Random logits in +-10 with planted 0.0, -0.0, +80 and -80; clip 1 of batch 0 has an empty truth, clip 2 of batch 1 has truth but
    no positive logit; every other clip has one box.  Half of the actions are the stand-in's arg-max, the others one class further."""
    g = np.random.default_rng(seed)
    net = ValNet(ncls)
    out = []
    for bi, n in enumerate(SIZES):
        data = g.random((n, 3, T, HW, HW))
        data[:, 0] = 0.5 + (2.0 * g.random((n, T, HW, HW)) - 1.0) * (10.0 / 160.0)
        msk = np.zeros((n, 1, T, HW, HW), np.float64)
        for i in range(n):
            h, w = int(g.integers(3, 10)), int(g.integers(3, 10))
            y0, x0 = int(g.integers(0, HW - h + 1)), int(g.integers(0, HW - w + 1))
            msk[i, 0, :, y0:y0 + h, x0:x0 + w] = 1.0
            # planted values, inside and outside the truth: (channel 0, channel 1) -> logit
            for t, (c0, c1) in enumerate(((0.5, 0.0), (0.5, 0.9), (1.0, 0.0), (0.0, 0.0), (1.0, 0.9), (0.0, 0.9))):
                for (yy, xx) in ((y0, x0), ((y0 + h) % HW, (x0 + w) % HW)):
                    data[i, 0, t, yy, xx], data[i, 1, t, yy, xx] = c0, c1
        if bi == 0:
            msk[1] = 0.0                                               # empty truth: IOU2 is NaN, validate leaves the clip out
        if bi == 1:
            data[2, 0] = 0.5 - g.random((T, HW, HW)) * (10.0 / 160.0) - 1e-3     # truth, but no positive logit: IoU 0
            data[2, 1] = 0.0
        with torch.no_grad():
            _seg, pred, _ = net(torch.from_numpy(data))
        top = pred.argmax(1).numpy()
        action = np.where(np.arange(n) % 2 == 0, top, (top + 1) % ncls).astype(np.float32).reshape(n, 1)
        out.append({"data": data, "loc_msk": msk, "action": action})
    return out
