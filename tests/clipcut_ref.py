"""The clip cut of csrc/evalclips.hip (pc_eval_clips_from_u8, pc_clips_from_u8, pc_clips_from_u8_views: one kernel) restated in numpy, shared
by tests/test_detect_kernels_gpu.py and tests/test_detect_views_kernels_gpu.py so that comparing one entry with another is not all that pins
them.  A byte becomes float32(byte / 255.0 in float64) through a 256-entry table, as in the kernel; frame k of a clip is video frame
start + f_skip * k, all zeros at or past F; a flipped view is the crop mirrored on the width axis; the fourth channel is 0."""
import numpy as np

LUT = (np.arange(256) / 255.0).astype(np.float32)


def cut(video, views, S, starts, truth=None, f_skip=2):
    """video uint8 [F,H,W,3], views [(h0, w0, flip)] -> data float32 [V, n, 8, S, S, 4]; with truth uint8 [F,H,W] -> (data, gt float32
    [V, n, 8, S, S]), the truth values themselves."""
    F = video.shape[0]
    data = np.zeros((len(views), len(starts), 8, S, S, 4), np.float32)
    gt = np.zeros(data.shape[:5], np.float32)
    for v, (h0, w0, fl) in enumerate(views):
        for c, s in enumerate(starts):
            for k in range(8):
                f = s + f_skip * k
                if f >= F:
                    continue
                crop = LUT[video[f, h0:h0 + S, w0:w0 + S]]
                data[v, c, k, :, :, :3] = crop[:, ::-1] if fl else crop
                if truth is not None:
                    t = truth[f, h0:h0 + S, w0:w0 + S].astype(np.float32)
                    gt[v, c, k] = t[:, ::-1] if fl else t
    return data if truth is None else (data, gt)


def same_bits(got, want):
    """A device float32 tensor against a numpy float32 array of as many elements: the same int32 bit patterns, -0.0 and all."""
    return np.array_equal(got.detach().cpu().contiguous().view(-1).numpy().view(np.int32), np.ascontiguousarray(want).reshape(-1).view(np.int32))
