"""GPU: the max-pool kernels (forward / backward) and pc_act_bwd, bit for bit.

Pools: a float32 CPU reference that scans the taps in (kt, kh, kw) order with a strict `>` from -inf (a padding tap contributes 0 and
index 255) and, backward, adds the windows of an input position in ascending (to, ho, wo) order with the old dx last.  Float32 compares,
selects and single additions in a fixed order have one result, so the comparison is torch.equal.  The shapes walk every compile-time window
form and the generic body, channel-slice strides, odd sizes, and block counts that are no multiple of 8 (the block -> work remap).

pc_act_bwd: dz is the torch expression (bit-equal for ReLU / none, 2 ulp for sigmoid); the bias gradient is within
4 * 2^-24 * sum|dz| + 2^-24 * |sum| of a float64 sum (fp32 runs of four rows flushed into double, plus the final rounding).

Every output is prefilled with a canary, the padding channels of sliced outputs must keep it, and every case runs twice to equal bits."""
import pytest
import torch

from picons_amd import capi, desc, ops, spec

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


POOL_CASES = [
    # k, s, N, (T, H, W), C, ldi, ldo
    pytest.param((1, 3, 3), (1, 2, 2), 3, (2, 9, 7), 8, 12, 8, id="133s122-odd-ldi12"),
    pytest.param((3, 3, 3), (2, 1, 1), 2, (3, 6, 5), 24, 24, 40, id="333s211-C24-ldo40"),
    pytest.param((3, 3, 3), (1, 1, 1), 2, (1, 5, 6), 16, 16, 16, id="333s111-T1"),
    pytest.param((3, 3, 3), (1, 1, 1), 2, (2, 5, 6), 16, 16, 16, id="333s111-T2"),
    pytest.param((3, 1, 1), (1, 1, 1), 1, (4, 3, 3), 4, 4, 4, id="311-generic"),
    pytest.param((3, 3, 3), (1, 1, 1), 5, (2, 28, 28), 64, 64, 64, id="333s111-280rows"),
    pytest.param((1, 3, 3), (1, 2, 2), 16, (4, 112, 112), 4, 4, 4, id="133s122-13MB"),
]


@pytest.mark.parametrize("ints", [False, True], ids=["random", "ints"])
@pytest.mark.parametrize("k,s,N,thw,C,ldi,ldo", POOL_CASES)
def test_pool_bits(k, s, N, thw, C, ldi, ldo, ints):
    g = torch.Generator().manual_seed(11)
    othw, pads = _pool_geometry(thw, k, s)
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


def _ulps(a, b):
    """distance of two float32 tensors in units in the last place (sign-magnitude -> ordered integers)"""
    def ordered(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (ordered(a) - ordered(b)).abs().max().item()


def _ref_act(dy, y, act):
    if act == capi.ACT_RELU:
        return torch.where(y > 0, dy, torch.zeros(()))
    if act == capi.ACT_SIGMOID:
        return dy * y * (1 - y)
    return dy.clone()


ACT_SHAPES = [
    # rows, C, lddy, ldy, lddz
    pytest.param(37, 4, 4, 4, 4, id="37x4"),
    pytest.param(1029, 24, 40, 40, 40, id="1029x24-ld40"),
    pytest.param(40003, 64, 128, 128, 64, id="40003x64-ld128"),
]


def _check_dbias(got, dz_ref, what):
    s64 = dz_ref.double().sum(0)
    bound = 4 * 2.0 ** -24 * dz_ref.double().abs().sum(0) + 2.0 ** -24 * s64.abs()
    err = (got.double() - s64).abs()
    assert (err <= bound).all(), "%s: bias gradient off by %.3e (bound %.3e)" % (what, err.max().item(), bound[err.argmax()].item())


@pytest.mark.parametrize("act", [capi.ACT_NONE, capi.ACT_RELU, capi.ACT_SIGMOID], ids=["none", "relu", "sigmoid"])
@pytest.mark.parametrize("rows,C,lddy,ldy,lddz", ACT_SHAPES)
def test_act_bwd(rows, C, lddy, ldy, lddz, act):
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(rows, C, generator=g)
    y = torch.rand(rows, C, generator=g) if act == capi.ACT_SIGMOID else torch.relu(torch.randn(rows, C, generator=g))
    old = torch.randn(C, generator=g)
    dz_ref = _ref_act(dy, y, act)
    dyd, yd = _sliced(dy, lddy), _sliced(y, ldy)

    def run(with_dz, dbias_mode, inplace=False):
        """-> (dz or None, dbias or None) on the CPU; twice, to equal bits"""
        outs = []
        for _ in range(2):
            src = _sliced(dy, lddy) if inplace else dyd
            dz = src if inplace else (torch.full((rows, lddz), CANARY, device=DEV) if with_dz else None)
            db = None if dbias_mode is None else (old.to(DEV) if dbias_mode == "accum" else torch.full((C,), CANARY, device=DEV))
            ops.act_bwd(src, lddy, yd, ldy, act, C, rows, dz, lddy if inplace else lddz, db, accum=dbias_mode == "accum")
            outs.append((None if dz is None else dz.cpu(), None if db is None else db.cpu()))
        for a, b in zip(*outs):
            assert (a is None and b is None) or torch.equal(a, b)
        return outs[0]

    def check_dz(dz, what):
        if act == capi.ACT_SIGMOID:
            assert _ulps(dz[:, :C], dz_ref) <= 2, what
        else:
            assert torch.equal(dz[:, :C], dz_ref), what
        assert (dz[:, C:] == CANARY).all(), what + ": padding channels of dz written"

    dz, fresh = run(True, "fresh")
    check_dz(dz, "dz with a fresh bias gradient")
    _check_dbias(fresh, dz_ref, "fresh")
    dz, acc = run(True, "accum")
    check_dz(dz, "dz with an accumulated bias gradient")
    assert torch.equal(acc, old + fresh), "accumulated bias gradient = old + the fresh one"
    dz, none = run(True, None)
    check_dz(dz, "dz alone")
    assert none is None
    _dz, only = run(False, "fresh")
    assert torch.equal(only, fresh), "bias gradient alone"
    if act == capi.ACT_RELU:
        dz, db = run(True, "fresh", inplace=True)
        check_dz(dz, "dz in place of dy")
        assert torch.equal(db, fresh)
    if act == capi.ACT_NONE:           # dz == dy without an activation: nothing to write, the sums alone
        dz, db = run(True, "fresh", inplace=True)
        assert torch.equal(dz[:, :C], dy) and (dz[:, C:] == CANARY).all() and torch.equal(db, fresh)
    assert torch.equal(dyd.cpu()[:, :C], dy) and torch.equal(yd.cpu()[:, :C], y), "an input was written"
