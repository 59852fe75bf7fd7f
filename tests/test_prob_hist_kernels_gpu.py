"""GPU: pc_prob_truth_hist (csrc/probhist.hip) through ops.prob_truth_hist, equal to the numpy restatement (tests/prob_hist_ref.py) to the
integer.  `out` and the workspace are filled with canaries in front of every call -- nothing has to be zeroed, and frames outside f0 / nf keep
theirs.  The shapes: odd H * W (frames at every 2-byte phase of an 8-byte word: the wide load and the element loads, tail groups), a frame of
several blocks (the fold adds partials) and 1080 x 1920 (the cap of 64 blocks a frame).  The words: one (the lowest, the highest, a half),
the default 19, 64 (1..64, and 64 spread over the range).  The probabilities: noise, coarse blocks, every word and its two neighbours
planted, all 0, all 65535; the truth: noise, blocks, all zero, all 255."""
import numpy as np
import pytest
import torch

from picons_amd import detect, ops

from tests import prob_hist_ref as ref

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (5, 120, 136), (1, 1080, 1920)]
WORDS = {"lowest": [1], "highest": [65535], "half": [32768], "default19": detect.threshold_words().tolist(), "1..64": list(range(1, 65)),
         "spread64": [1] + list(range(1000, 63000, 1000)) + [65535]}
CANARY = -1515870811                                                                         # 0xa5a5a5a5
_cache = {}


def _specials():
    v = np.concatenate([np.asarray(w, np.int64) + d for w in WORDS.values() for d in (-1, 0, 1)] + [np.array([0, 65535])])
    return np.unique(np.clip(v, 0, 65535)).astype(np.uint16)


def _maps(shape):
    """(prob, truth) of a shape on the host and on the device, made once.  Upper half of a frame: coarse blocks (long runs of one cell), lower
    half: noise (the cell changes at every pixel) with every word of WORDS and its neighbours planted, half of the noise a probability of 0.
    On the device prob lies at an odd ELEMENT offset and truth at an odd byte offset of their allocations."""
    if shape not in _cache:
        F, H, W = shape
        rng = np.random.default_rng(sum(shape))
        sp = _specials()
        noise = rng.integers(0, 65536, shape).astype(np.uint16)
        noise[rng.random(shape) < 0.5] = 0
        plant = rng.random(shape) < 0.3
        noise[plant] = sp[rng.integers(0, sp.size, int(plant.sum()))]
        coarse = sp[rng.integers(0, sp.size, (F, -(-H // 7), -(-W // 13)))]
        blocks = np.repeat(np.repeat(coarse, 7, axis=1), 13, axis=2)[:, :H, :W]
        upper = np.arange(H)[None, :, None] < H // 2
        prob = np.ascontiguousarray(np.where(upper, blocks, noise))
        tn = (rng.random(shape) < 0.4) * rng.integers(1, 256, shape)
        tc = (rng.random((F, -(-H // 5), -(-W // 11))) < 0.4) * rng.integers(1, 256, (F, -(-H // 5), -(-W // 11)))
        tb = np.repeat(np.repeat(tc, 5, axis=1), 11, axis=2)[:, :H, :W]
        truth = np.ascontiguousarray(np.where(np.arange(W)[None, None, :] < W // 2, tb, tn).astype(np.uint8))
        pbuf = torch.zeros(prob.size + 8, dtype=torch.int16, device="cuda")
        pbuf[1:1 + prob.size].copy_(torch.from_numpy(prob.view(np.int16)).reshape(-1))
        tbuf = torch.zeros(truth.size + 8, dtype=torch.uint8, device="cuda")
        tbuf[3:3 + truth.size].copy_(torch.from_numpy(truth).reshape(-1))
        _cache[shape] = (prob, truth, pbuf[1:1 + prob.size].view(shape), tbuf[3:3 + truth.size].view(shape))
    return _cache[shape]


def _call(prob, truth, words, f0=0, nf=None):
    F, H, W = prob.shape
    N = len(words)
    out = torch.full((F, 2, N + 1), CANARY, dtype=torch.int32, device="cuda")
    ws = torch.full((ops.prob_truth_hist_ws_bytes(F - f0 if nf is None else nf, H, W, N),), 0xa5, dtype=torch.uint8, device="cuda")
    got = ops.prob_truth_hist(prob, truth, words, f0=f0, nf=nf, out=out, ws=ws)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(WORDS))
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement(shape, name):
    hp, ht, dp, dt = _maps(shape)
    words = WORDS[name]
    assert dp.data_ptr() % 4 == 2 and dt.data_ptr() % 2 == 1
    want = ref.hist(hp, ht, words)
    got = _call(dp, dt, words)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(shape[0], -1).sum(axis=1), np.full(shape[0], shape[1] * shape[2]))
    assert np.array_equal(_call(dp, dt, words), got)         # the same bits from a second run
    assert np.array_equal(detect.sweep_counts(got), ref.sweep_counts(want))


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 120, 136)])
def test_a_sub_range_leaves_the_other_frames_alone(shape):
    hp, ht, dp, dt = _maps(shape)
    F = shape[0]
    for name in ("half", "default19", "1..64"):
        got = _call(dp, dt, WORDS[name], f0=1, nf=F - 2)
        assert (got[0] == CANARY).all() and (got[F - 1] == CANARY).all()
        assert np.array_equal(got[1:F - 1], ref.hist(hp[1:F - 1], ht[1:F - 1], WORDS[name]))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31), (5, 120, 136), (1, 1080, 1920)])
def test_constant_maps(shape):
    F, H, W = shape
    for pv, tv, name in ((0, 0, "half"), (0, 0, "1..64"), (65535, 255, "highest"), (65535, 0, "spread64"), (0, 255, "default19"), (65535, 255, "1..64"),
                         (32767, 1, "half"), (32768, 0, "half"), (64, 7, "1..64"), (63, 0, "1..64"), (3276, 255, "default19"), (3277, 0, "default19")):
        words = WORDS[name]
        prob = torch.full(shape, pv - 65536 if pv > 32767 else pv, dtype=torch.int16, device="cuda")
        truth = torch.full(shape, tv, dtype=torch.uint8, device="cuda")
        got = _call(prob, truth, words)
        want = np.zeros((F, 2, len(words) + 1), np.int32)
        want[:, int(tv != 0), sum(1 for w in words if w <= pv)] = H * W
        assert np.array_equal(got, want), (pv, tv, name)
        if H * W <= 1 << 16:                                 # (the restatement agrees with the table written out above)
            assert np.array_equal(want, ref.hist(np.full(shape, pv, np.uint16), np.full(shape, tv, np.uint8), words))


def test_frames_at_every_phase_of_an_eight_byte_word():
    """H * W = 35 is odd and 3 mod 4: the four frames start 0, 6, 4 and 2 bytes into an 8-byte word from an aligned base, and elsewhere from a
    base moved by one, two and three elements."""
    hp, ht, _dp, dt = _maps((3, 5, 7))
    hp4 = np.concatenate([hp, hp[:1]])
    ht4 = np.concatenate([ht, ht[:1]])
    want = ref.hist(hp4, ht4, WORDS["default19"])
    for off in range(4):
        buf = torch.zeros(hp4.size + 8, dtype=torch.int16, device="cuda")
        buf[off:off + hp4.size].copy_(torch.from_numpy(hp4.view(np.int16)).reshape(-1))
        got = _call(buf[off:off + hp4.size].view(hp4.shape), torch.from_numpy(ht4).cuda(), WORDS["default19"])
        assert np.array_equal(got, want), off


def test_a_fresh_out_is_zero_filled_and_arguments_are_checked():
    hp, ht, dp, dt = _maps((3, 5, 7))
    words = WORDS["default19"]
    got = ops.prob_truth_hist(dp, dt, words, f0=1, nf=1)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 2, 20)
    g = got.cpu().numpy()
    assert (g[0] == 0).all() and (g[2] == 0).all() and np.array_equal(g[1:2], ref.hist(hp[1:2], ht[1:2], words))
    assert np.array_equal(ops.decode_prob_truth_hist(got, 19), g)
    assert np.array_equal(ops.prob_truth_hist(dp, dt, np.asarray(words, np.uint16)).cpu().numpy(), ref.hist(hp, ht, words))      # words as an array
    if hasattr(torch, "uint16"):
        assert np.array_equal(ops.prob_truth_hist(dp.view(torch.uint16), dt, words).cpu().numpy(), ref.hist(hp, ht, words))
    out = torch.zeros(3, 2, 20, dtype=torch.int32, device="cuda")
    for kw in (dict(words=[]), dict(words=[0]), dict(words=[0, 5]), dict(words=[5, 5]), dict(words=[9, 5]), dict(words=[65536]), dict(words=[-1, 5]),
               dict(words=list(range(1, 66))), dict(words=[0.5]), dict(words=[[1, 2]]), dict(words=5), dict(words=None),
               dict(f0=-1), dict(nf=0), dict(f0=1, nf=3), dict(f0=3),
               dict(out=out[:2]), dict(out=out.float()), dict(out=out.cpu()), dict(out=out[:, :, :19]), dict(ws=torch.zeros(8, dtype=torch.uint8, device="cuda")),
               dict(ws=torch.zeros(4096, dtype=torch.int32, device="cuda")), dict(ws=torch.zeros(4096, dtype=torch.uint8))):
        args = dict(words=words)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.prob_truth_hist(dp, dt, **args)
    for bad_p, bad_t in ((dp.cpu().numpy(), dt), (dp, dt[:2]), (dp.to(torch.int32), dt), (dp.to(torch.uint8), dt), (dp, dt.to(torch.int16)),
                         (dp[:, :, :5], dt[:, :, :5]), (dp[0], dt[0]), (dp.cpu(), dt), (dp, dt.cpu())):
        with pytest.raises(ValueError):
            ops.prob_truth_hist(bad_p, bad_t, words)
