"""GPU: pc_map_crosstab (csrc/crosstab.hip) through ops.map_crosstab, equal to the numpy restatement (tests/map_crosstab_ref.py) to the
integer.  `out` and the workspace are filled with canaries in front of every call -- nothing has to be zeroed, and frames outside f0 / nf keep
theirs.  The shapes: odd H * W (the two sides sit differently in their dwords, tail groups), a small and a full-size frame (several blocks a
frame: the fold adds partials), and 1080 x 1920 (the cap of 64 blocks a frame).  The bytes: 0, 1, values at and just above P and A, 255; noise
(the pair changes at every pixel) and blocks (long runs of one pair); all-zero and all-foreground maps."""
import numpy as np
import pytest
import torch

from picons_amd import ops

from tests import map_crosstab_ref as ref

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 31), (5, 120, 136), (40, 240, 320), (1, 1080, 1920)]
PS, AS = (1, 8, 32), (1, 3, 32)
PALETTE = np.array([0, 0, 0, 0, 0, 1, 1, 2, 3, 4, 8, 9, 32, 33, 34, 200, 255], np.uint8)      # 2, 9, 33 / 2, 4, 33: just above P / A
CANARY = -1515870811                                                                         # 0xa5a5a5a5
_cache = {}


def _side(rng, shape):
    F, H, W = shape
    noise = PALETTE[rng.integers(0, PALETTE.size, shape)]
    coarse = PALETTE[rng.integers(0, PALETTE.size, (F, -(-H // 7), -(-W // 13)))]
    blocks = np.repeat(np.repeat(coarse, 7, axis=1), 13, axis=2)[:, :H, :W]
    return np.ascontiguousarray(np.where(np.arange(H)[None, :, None] < H // 2, blocks, noise))


def _maps(shape):
    """(pred, truth) of a shape on the host and on the device, made once.  On the device both lie at odd byte offsets of one allocation each,
    one byte apart from each other modulo 4."""
    if shape not in _cache:
        rng = np.random.default_rng(sum(shape))
        host = (_side(rng, shape), _side(rng, shape))
        dev = []
        for off, m in zip((1, 2), host):
            buf = torch.zeros(m.size + 8, dtype=torch.uint8, device="cuda")
            buf[off:off + m.size].copy_(torch.from_numpy(m).reshape(-1))
            dev.append(buf[off:off + m.size].view(shape))
        _cache[shape] = host + tuple(dev)
    return _cache[shape]


def _call(pred, truth, P, A, f0=0, nf=None):
    F, H, W = pred.shape
    out = torch.full((F, P + 2, A + 2), CANARY, dtype=torch.int32, device="cuda")
    ws = torch.full((ops.map_crosstab_ws_bytes(F - f0 if nf is None else nf, H, W, P, A),), 0xa5, dtype=torch.uint8, device="cuda")
    got = ops.map_crosstab(pred, truth, P, A, f0=f0, nf=nf, out=out, ws=ws)
    assert got is out
    return out.cpu().numpy()


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("shape", SHAPES)
def test_tables_equal_the_restatement(shape, P, A):
    hp, ht, dp, dt = _maps(shape)
    assert dp.data_ptr() % 4 != dt.data_ptr() % 4
    want = ref.crosstab(hp, ht, P, A)
    got = _call(dp, dt, P, A)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got.reshape(shape[0], -1).sum(axis=1), np.full(shape[0], shape[1] * shape[2]))
    assert np.array_equal(_call(dp, dt, P, A), got)          # the same bits from a second run


@pytest.mark.parametrize("shape", [(3, 5, 7), (5, 120, 136), (40, 240, 320)])
def test_a_sub_range_leaves_the_other_frames_alone(shape):
    hp, ht, dp, dt = _maps(shape)
    F = shape[0]
    for P, A in ((1, 1), (8, 3)):
        got = _call(dp, dt, P, A, f0=1, nf=F - 2)
        assert (got[0] == CANARY).all() and (got[F - 1] == CANARY).all()
        assert np.array_equal(got[1:F - 1], ref.crosstab(hp[1:F - 1], ht[1:F - 1], P, A))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 33, 31), (5, 120, 136), (1, 1080, 1920)])
def test_all_zero_and_all_foreground_maps(shape):
    F, H, W = shape
    for pv, tv, P, A in ((0, 0, 1, 1), (0, 0, 32, 32), (1, 1, 1, 1), (255, 255, 8, 3), (0, 7, 8, 3), (9, 0, 8, 32), (2, 4, 1, 3), (32, 32, 32, 32)):
        pred = torch.full(shape, pv, dtype=torch.uint8, device="cuda")
        truth = torch.full(shape, tv, dtype=torch.uint8, device="cuda")
        got = _call(pred, truth, P, A)
        want = np.zeros((F, P + 2, A + 2), np.int32)
        want[:, min(pv, P + 1), min(tv, A + 1)] = H * W
        assert np.array_equal(got, want), (pv, tv, P, A)
        if H * W <= 1 << 16:                                 # (the restatement agrees with the table written out above)
            assert np.array_equal(want, ref.crosstab(np.full(shape, pv, np.uint8), np.full(shape, tv, np.uint8), P, A))


def test_a_fresh_out_is_zero_filled_and_arguments_are_checked():
    hp, ht, dp, dt = _maps((3, 5, 7))
    got = ops.map_crosstab(dp, dt, 8, 3, f0=1, nf=1)
    assert got.dtype == torch.int32 and tuple(got.shape) == (3, 10, 5)
    g = got.cpu().numpy()
    assert (g[0] == 0).all() and (g[2] == 0).all() and np.array_equal(g[1:2], ref.crosstab(hp[1:2], ht[1:2], 8, 3))
    assert np.array_equal(ops.decode_map_crosstab(got, 8, 3), g)
    out = torch.zeros(3, 10, 5, dtype=torch.int32, device="cuda")
    for kw in (dict(P=0), dict(P=33), dict(A=0), dict(A=33), dict(f0=-1), dict(nf=0), dict(f0=1, nf=3), dict(f0=3),
               dict(out=out[:2]), dict(out=out.float()), dict(out=out.cpu()), dict(ws=torch.zeros(8, dtype=torch.uint8, device="cuda")),
               dict(ws=torch.zeros(4096, dtype=torch.int32, device="cuda"))):
        args = dict(P=8, A=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.map_crosstab(dp, dt, **args)
    for bad_p, bad_t in ((dp.cpu().numpy(), dt), (dp, dt[:2]), (dp.to(torch.int32), dt), (dp[:, :, :5], dt[:, :, :5]), (dp[0], dt[0])):
        with pytest.raises(ValueError):
            ops.map_crosstab(bad_p, bad_t, 8, 3)
