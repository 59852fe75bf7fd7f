"""GPU: the register-tile max-pool kernels -- the 3x3x3 windows with stride 1 along h and w, (1,1,1) and (2,1,1) -- bit for bit.

The reference is the float32 CPU scan of tests/test_pool_actbwd_gpu.py, restated here: taps in (kt, kh, kw) order with a strict `>` from
-inf, a padding tap 0 with index 255; backward the windows of an input position in ascending (to, ho, wo) order with the old dx last.
Compares, selects and single float32 additions in a fixed order have one result, so the comparison is torch.equal.

A thread of these kernels owns a tile of four positions (2 x 2 outputs forward, four input positions along w backward), so the widths run
below a tile, a tile plus one and odd, the heights 1 and 4; C / 4 does not divide 256, so a block's 256 items start in the middle of a row;
N makes at least 9 blocks in both directions and a block count that is no multiple of 8 (the block -> work remap).  Every output is
prefilled with a canary, the padding channels of sliced tensors must keep it, and every case runs twice to equal bits."""
import pytest
import torch

from picons_amd import desc, ops, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -777.25


def _pool_geometry(thw, k, s):
    othw = [spec.same_out(thw[i], k[i], s[i]) for i in range(3)]
    pads = [spec.same_pad(thw[i], k[i], s[i]) for i in range(3)]
    return othw, pads


def _ref_pool_fwd(x, k, s, othw, pads):
    """x (N, T, H, W, C) float32 cpu -> y, argmax (uint8)"""
    N, T, H, W, C = x.shape
    xp = torch.zeros(N, T + sum(pads[0]), H + sum(pads[1]), W + sum(pads[2]), C)
    inside = torch.zeros(xp.shape[1:4], dtype=torch.bool)
    f = [p[0] for p in pads]
    xp[:, f[0]:f[0] + T, f[1]:f[1] + H, f[2]:f[2] + W] = x
    inside[f[0]:f[0] + T, f[1]:f[1] + H, f[2]:f[2] + W] = True
    best = torch.full((N, *othw, C), float("-inf"))
    idx = torch.full((N, *othw, C), 255, dtype=torch.int64)
    tap = 0
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                sl = (slice(a, a + (othw[0] - 1) * s[0] + 1, s[0]), slice(b, b + (othw[1] - 1) * s[1] + 1, s[1]), slice(c, c + (othw[2] - 1) * s[2] + 1, s[2]))
                v = xp[(slice(None),) + sl]
                code = torch.where(inside[sl], torch.tensor(tap), torch.tensor(255))[None, ..., None]
                upd = v > best
                best = torch.where(upd, v, best)
                idx = torch.where(upd, code.expand_as(idx), idx)
                tap += 1
    return best, idx.to(torch.uint8)


def _ref_pool_bwd(dy, am, old, k, s, thw, othw, pads):
    """Ascending (to, ho, wo) for one input position is descending (kt, kh, kw): one window per tap."""
    N, C = dy.shape[0], dy.shape[-1]
    T, H, W = thw
    gp = torch.zeros(N, T + sum(pads[0]), H + sum(pads[1]), W + sum(pads[2]), C)
    f = [p[0] for p in pads]
    zero = torch.zeros(())
    for a in reversed(range(k[0])):
        for b in reversed(range(k[1])):
            for c in reversed(range(k[2])):
                tap = (a * k[1] + b) * k[2] + c
                sl = (slice(None), slice(a, a + (othw[0] - 1) * s[0] + 1, s[0]), slice(b, b + (othw[1] - 1) * s[1] + 1, s[1]),
                      slice(c, c + (othw[2] - 1) * s[2] + 1, s[2]))
                gp[sl] = gp[sl] + torch.where(am == tap, dy, zero)
    g = gp[:, f[0]:f[0] + T, f[1]:f[1] + H, f[2]:f[2] + W]
    return g + old if old is not None else g.clone()


def _sliced(data, ld):
    """(..., C) cpu -> cuda buffer (..., ld) of canaries with the data in its first C channels"""
    buf = torch.full((*data.shape[:-1], ld), CANARY, device=DEV)
    buf[..., :data.shape[-1]] = data.to(DEV)
    return buf


def _blocks(n_tiles, C):
    return -(-n_tiles * (C // 4) // 256)


def _pick_n(thw, othw, C):
    """the smallest N with at least 9 blocks of 256 (tile, channel quad) items, no multiple of 8, forward (2 x 2 outputs) and backward (four
    input positions along w)"""
    T, H, W = thw
    for N in range(1, 4000):
        nf = _blocks(N * othw[0] * -(-othw[1] // 2) * -(-othw[2] // 2), C)
        nb = _blocks(N * T * H * -(-W // 4), C)
        if nf >= 9 and nb >= 9 and nf % 8 and nb % 8:
            return N
    raise AssertionError("no batch size gives the block counts the test wants")


# T, H, W, C, ldi, ldo: every W of {1, 2, 3, 5, 9}, H of {1, 4}, T of {1, 2, 3}, C of {4, 20, 36}; ldi > C and ldo > C
SHAPES = [
    pytest.param(1, 1, 1, 36, 36, 36, id="T1-1x1-C36"),
    pytest.param(1, 4, 2, 20, 20, 24, id="T1-4x2-C20-ldo24"),
    pytest.param(2, 1, 3, 4, 8, 4, id="T2-1x3-C4-ldi8"),
    pytest.param(2, 4, 5, 36, 40, 36, id="T2-4x5-C36-ldi40"),
    pytest.param(3, 4, 9, 20, 28, 32, id="T3-4x9-C20-ldi28-ldo32"),
    pytest.param(3, 1, 9, 4, 4, 12, id="T3-1x9-C4-ldo12"),
    pytest.param(1, 4, 5, 4, 4, 4, id="T1-4x5-C4"),
    pytest.param(3, 4, 3, 36, 36, 44, id="T3-4x3-C36-ldo44"),
]


@pytest.mark.parametrize("ints", [False, True], ids=["random", "ints"])
@pytest.mark.parametrize("st", [1, 2], ids=["s111", "s211"])
@pytest.mark.parametrize("T,H,W,C,ldi,ldo", SHAPES)
def test_pool_tile_bits(T, H, W, C, ldi, ldo, st, ints):
    k, s, thw = (3, 3, 3), (st, 1, 1), (T, H, W)
    g = torch.Generator().manual_seed(23)
    othw, pads = _pool_geometry(thw, k, s)
    N = _pick_n(thw, othw, C)
    if ints:        # ties everywhere, and windows whose values are all negative: the zero of a padding tap wins with index 255
        x = torch.randint(-2, 3, (N, *thw, C), generator=g).float()
        dy = torch.randint(-2, 3, (N, *othw, C), generator=g).float()
        old = torch.randint(-2, 3, (N, *thw, C), generator=g).float()
    else:
        x, dy, old = torch.randn(N, *thw, C, generator=g), torch.randn(N, *othw, C, generator=g), torch.randn(N, *thw, C, generator=g)
    y_ref, am_ref = _ref_pool_fwd(x, k, s, othw, pads)
    d = desc.pool(N, thw, C, ldi, othw, ldo, k, s, [p[0] for p in pads])
    xd = _sliced(x, ldi)
    runs = []
    for _ in range(2):
        y = torch.full((N, *othw, ldo), CANARY, device=DEV)
        am = torch.full((N, *othw, C), 77, device=DEV, dtype=torch.uint8)
        ops.maxpool_fwd(d, xd, y, am)
        runs.append((y.cpu(), am.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    y, am = runs[0]
    assert torch.equal(y[..., :C], y_ref), "forward values"
    assert torch.equal(am, am_ref), "forward argmax"
    assert (y[..., C:] == CANARY).all(), "forward wrote the padding channels of its output"
    assert torch.equal(xd.cpu()[..., :C], x) and (xd.cpu()[..., C:] == CANARY).all()
    if ints:
        assert (am_ref == 255).any(), "the integer case is there to make padding taps win"
    dyd, amd = _sliced(dy, ldo), am_ref.to(DEV)
    for accum in (0, 1):
        ref = _ref_pool_bwd(dy, am_ref, old if accum else None, k, s, thw, othw, pads)
        runs = []
        for _ in range(2):
            dx = _sliced(old, ldi)
            ops.maxpool_bwd(d, dyd, amd, dx, accum=bool(accum))
            runs.append(dx.cpu())
        assert torch.equal(runs[0], runs[1])
        assert torch.equal(runs[0][..., :C], ref), "backward, accum=%d" % accum
        assert (runs[0][..., C:] == CANARY).all(), "backward wrote the padding channels of dx"
    assert torch.equal(dyd.cpu()[..., :C], dy) and torch.equal(amd.cpu(), am_ref), "an input of the backward pass was written"
