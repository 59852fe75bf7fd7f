"""GPU: the three kernels of csrc/evalclips.hip at the smallest shapes that can still go wrong.  pc_eval_clips_from_u8 bit for bit against
the oracle's make_clips on (u8 crop) / 255. in float64, pc_truth_frame_flags against np.count_nonzero on the crop, pc_video_vote against
np.argmax(np.mean(p, axis=0))."""
import numpy as np
import pytest
import torch

from oracle import evalmetrics as oe
from picons_amd import evalstep, ops

pytestmark = pytest.mark.gpu
CANARY = 0x5A5AA5A5            # an int32 bit pattern (1.5e16 as float32) no kernel output equals


def _video(F, H, W, seed):
    rng = np.random.default_rng(seed)
    video = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    video[0, :, :, 0] = np.arange(H * W, dtype=np.int64).reshape(H, W) % 256          # every byte value, at known places
    truth = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), (F, H, W, 1))
    return video, truth


def _expected(video, truth, h0, w0, S, starts):
    """The oracle's clips of the cropped video for the given first frames: make_clips keeps a clip only if it has truth, so each start is cut from
    its own 16-frame window with the truth it has -- here every start is taken, kept or not, by building the clip the way make_clips does."""
    F = video.shape[0]
    vc = video[:, h0:h0 + S, w0:w0 + S] / 255.                    # float64, as the loader yields it
    tc = truth[:, h0:h0 + S, w0:w0 + S]
    data = np.zeros((len(starts), 8, S, S, 4), np.float32)
    gt = np.zeros((len(starts), 8, S, S), np.float32)
    for c, s in enumerate(starts):
        for k in range(8):
            f = s + 2 * k
            if f < F:
                data[c, k, :, :, :3] = vc[f]                      # the float32 cast of make_clips
                gt[c, k] = tc[f, :, :, 0]
    return data, gt


def _run(video, truth, h0, w0, S, starts):
    n = len(starts)
    pad = 64
    dbuf = torch.full((pad + n * 8 * S * S * 4 + pad,), CANARY, dtype=torch.int32, device="cuda")
    gbuf = torch.full((pad + n * 8 * S * S + pad,), CANARY, dtype=torch.int32, device="cuda")
    data, gt = dbuf[pad:-pad].view(torch.float32), gbuf[pad:-pad].view(torch.float32)
    dv, dt = torch.from_numpy(video).cuda(), torch.from_numpy(np.ascontiguousarray(truth[..., 0])).cuda()
    ops.eval_clips_from_u8(dv, dt, h0, w0, S, starts, 2, out=(data, gt))
    torch.cuda.synchronize()
    for buf in (dbuf, gbuf):                                       # canary words in front of and behind both outputs
        assert (buf[:pad] == CANARY).all() and (buf[-pad:] == CANARY).all()
    return data.view(n, 8, S, S, 4).cpu(), gt.view(n, 8, S, S).cpu()


CASES = [(1, 8, 8, 8, 0, 0), (3, 9, 11, 4, 2, 3), (17, 10, 12, 8, 1, 2), (40, 12, 12, 8, 0, 0)]


@pytest.mark.parametrize("F,H,W,S,h0,w0", CASES)
def test_eval_clips_equal_the_oracles_make_clips_bit_for_bit(F, H, W, S, h0, w0):
    video, truth = _video(F, H, W, 100 + F)
    starts = [i + j for i in range(0, F, 16) for j in (0, 1)]      # every window and phase: for F = 17, start 16 has one real frame, start 17 none
    if F == 17:
        assert starts == [0, 1, 16, 17]
    data, gt = _run(video, truth, h0, w0, S, starts)
    want_d, want_g = _expected(video, truth, h0, w0, S, starts)
    assert torch.equal(data, torch.from_numpy(want_d)) and torch.equal(gt, torch.from_numpy(want_g))
    assert (data[..., 3] == 0).all() and not np.signbit(data[..., 3].numpy()).any()           # the fourth channel is exactly 0
    assert set(np.unique(gt.numpy()).tolist()) <= {0.0, 1.0, 2.0, 255.0} and (gt == 255).any() == bool((want_g == 255).any())
    # the clips the oracle keeps are these, in this order
    vc = video[:, h0:h0 + S, w0:w0 + S] / 255.
    tc = truth[:, h0:h0 + S, w0:w0 + S]
    kept = [c for c, s in enumerate(starts) if want_g[c].sum() != 0]
    clips = oe.make_clips(vc, tc, 0)
    assert len(clips) == len(kept)
    for c, (v, b, _l) in zip(kept, clips):
        assert torch.equal(data[c, ..., :3], torch.from_numpy(v)) and torch.equal(gt[c], torch.from_numpy(b[..., 0]))


def test_eval_clips_32_clips_in_one_launch():
    F, H, W, S, h0, w0 = 17, 10, 12, 8, 1, 2
    video, truth = _video(F, H, W, 9)
    starts = ([0, 1, 16, 17] * 8)[:32]
    data, gt = _run(video, truth, h0, w0, S, starts)
    want_d, want_g = _expected(video, truth, h0, w0, S, starts)
    assert torch.equal(data, torch.from_numpy(want_d)) and torch.equal(gt, torch.from_numpy(want_g))
    assert (data[3::4] == 0).all() and (gt[3::4] == 0).all()       # start 17: no frame of the video


def test_every_byte_value_divides_as_float64_rounded_once():
    video = np.zeros((1, 16, 16, 3), np.uint8)
    video[0, :, :, 1] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    truth = np.ones((1, 16, 16, 1), np.uint8)
    data, _gt = _run(video, truth, 0, 0, 16, [0])
    want = (np.arange(256, dtype=np.float64) / 255.).astype(np.float32)
    assert np.array_equal(data[0, 0, :, :, 1].numpy().reshape(-1), want)


@pytest.mark.parametrize("F,H,W,S,h0,w0", CASES + [(5, 40, 44, 33, 3, 7)])
def test_truth_frame_flags_count_the_crop(F, H, W, S, h0, w0):
    _video_, truth = _video(F, H, W, 200 + F)
    truth = np.ascontiguousarray(truth[..., 0])
    truth[F // 2] = 0
    truth[F // 2, :h0, :] = 7; truth[F // 2, :, :w0] = 1; truth[F // 2, h0 + S:, :] = 1; truth[F // 2, :, w0 + S:] = 255     # only outside the crop
    buf = torch.full((8 + F + 8,), CANARY, dtype=torch.int32, device="cuda")
    flags = ops.truth_frame_flags(torch.from_numpy(truth).cuda(), h0, w0, S, buf[8:8 + F])
    torch.cuda.synchronize()
    want = np.count_nonzero(truth[:, h0:h0 + S, w0:w0 + S].reshape(F, -1), axis=1)
    assert np.array_equal(flags.cpu().numpy(), want) and want[F // 2] == 0
    assert (buf[:8] == CANARY).all() and (buf[8 + F:] == CANARY).all()
    if (h0, w0) != (0, 0) or S < H:
        assert truth[F // 2].any()


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("Cn", [21, 24])
def test_video_vote(n, Cn):
    rng = np.random.default_rng(n * 100 + Cn)
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    expect = 0
    for case in range(6):
        p = rng.standard_normal((n, Cn)).astype(np.float32)
        if case == 1:                                              # an exact tie: the first maximum wins
            p[:, 5] = 9.0; p[:, 17] = 9.0
        best = int(np.argmax(np.mean(p, axis=0)))
        assert best == evalstep.vote(p)
        if case == 1:
            assert best == 5
        label = best if case % 2 == 1 else (best + 1) % Cn         # a label that matches and one that does not, into ONE counter
        expect += int(label == best)
        ops.video_vote(torch.from_numpy(p).cuda(), label, count)
    assert int(count.item()) == expect == 3


def test_wrappers_refuse_bad_tensors_before_any_launch():
    v = torch.zeros(4, 12, 12, 3, dtype=torch.uint8, device="cuda")
    t = torch.zeros(4, 12, 12, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.eval_clips_from_u8(v.float(), t, 0, 0, 8, [0])
    with pytest.raises(ValueError):
        ops.eval_clips_from_u8(v, t[:3], 0, 0, 8, [0])
    with pytest.raises(ValueError):
        ops.eval_clips_from_u8(v, t, 0, 0, 8, [0, 1], out=(torch.zeros(8 * 8 * 8 * 4, device="cuda"), torch.zeros(2 * 8 * 8 * 8, device="cuda")))
    with pytest.raises(RuntimeError, match="outside"):
        ops.eval_clips_from_u8(v, t, 5, 0, 8, [0])                # the library's own check: PC_E_ARG, no launch
    with pytest.raises(RuntimeError, match="clips outside"):
        ops.eval_clips_from_u8(v, t, 0, 0, 8, list(range(33)))
    with pytest.raises(ValueError):
        ops.truth_frame_flags(t.float(), 0, 0, 8)
    with pytest.raises(ValueError):
        ops.video_vote(torch.zeros(3, 24, device="cuda").double(), 0, torch.zeros(1, dtype=torch.int32, device="cuda"))
