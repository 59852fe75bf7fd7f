"""The view merge of pc_detect_frames_views restated in numpy float32, shared by tests/test_detect_views_kernels_gpu.py and
tests/test_detect_views_gpu.py.  Per full-frame pixel the views that cover it are visited in table order: the first value is taken as it is
(no zero start: -0.0 and NaN pass through), later ones are added in float32, and the sum is divided once by float32(count) when count > 1.
numpy's float32 add and divide are IEEE round-to-nearest, as __fadd_rn / __fdiv_rn are, so the merged logit is reproduced bit for bit."""
import numpy as np
import torch


def real_frames(starts, F, f_skip=2):
    """[(clip, frame of the clip, video frame)] of the clips' frames below F."""
    return [(c, k, s + f_skip * k) for c, s in enumerate(starts) for k in range(8) if s + f_skip * k < F]


class Merge:
    """Accumulates launches into merged logits [F,H,W] float32 and cover counts [F,H,W]."""

    def __init__(self, F, H, W, S):
        self.F, self.H, self.W, self.S = F, H, W, S
        self.acc = np.zeros((F, H, W), np.float32)
        self.num = np.zeros((F, H, W), np.int32)

    def add(self, x, views, starts):
        """x: float32 [V, n, 8, S, S] (view, clip, frame of the clip), the clips cut at `starts`."""
        S = self.S
        x = np.asarray(x, np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for c, k, f in real_frames(starts, self.F):
                for v, (h0, w0, fl) in enumerate(views):
                    t = x[v, c, k][:, ::-1] if fl else x[v, c, k]
                    a, m = self.acc[f, h0:h0 + S, w0:w0 + S], self.num[f, h0:h0 + S, w0:w0 + S]
                    a[...] = np.where(m > 0, (a + t).astype(np.float32), t)
                    m += 1

    def merged(self):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = (self.acc / np.maximum(self.num, 1).astype(np.float32)).astype(np.float32)
        return np.where(self.num > 1, q, self.acc)

    def masks(self):
        """uint8 [F,H,W]: the evaluator's predicate as the reference states it (fp32 sigmoid(x) >= 0.5 on the host) on the merged logit of the
        covered pixels, 0 where no view covers."""
        pos = (torch.sigmoid(torch.from_numpy(self.merged())) >= 0.5).numpy()
        return (pos & (self.num > 0)).astype(np.uint8)


def box_of(mask2d):
    ys, xs = np.nonzero(mask2d)
    return (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if ys.size else (0, 0, 0, 0)


def score_refs(merged2d, mask2d):
    """(float64 mean sigmoid, fp32 torch mean sigmoid) over the positive pixels of one frame."""
    sel = torch.from_numpy(merged2d[mask2d.astype(bool)])
    return float((1.0 / (1.0 + torch.exp(-sel.double()))).mean()), float((1.0 / (1.0 + torch.exp(-sel))).mean())
