"""PC_F_BKMAJOR: the bf16-split conv kernel reading K-major weight planes [g][Ci][taps][N] -- a layer's FORWARD planes, read as they are by
its input gradient (csrc/conv_x6.hip: the B tile is fetched [32 k][BN] and transposed by ds_read_b64_tr_b16).  The products and their order
are those of the launch fed with the transposed copy [g][N][taps][Ci], so the bar is bit-equality with that launch, with and without the
tail split; one case on small integers, where every sum is exact, is also held to a float64 sum (a wrong k pairing between the A and B
fragments changes that sum and cannot hide behind rounding).

Shapes: grouped 1 x 9 x 1 input gradients (mirrored taps, sample-fastest rows) with a per-group weight stride, 96 contraction channels =
3 chunks per tap and 27 in all (the two-buffer ring wraps on an odd count; >= 12 chunks per K slice), 28 gathered rows per sample.  The
first is the one the spectral PrimaryCaps weight producer feeds (pc_wspec_master_planes, both layouts); the other two are the smallest
launches for which pc_x6_tile picks the two tiles the PrimaryCaps input gradient takes at 2 .. 8 clips (a launch that fills no round of
resident blocks gets 64 x 64)."""
import ctypes as C

import pytest
import torch

from picons_amd import capi, desc, ops

DEV = "cuda"
KY, H = 9, 28
OH = H - KY + 1


def _dgrad(G, nf, K, N, fwd_planes):
    """One descriptor (stride 1: one parity class) of the grouped input gradient: [G * nf][OH][K] -> [G * nf][H][N]."""
    (d,) = desc.transposed_classes(G * nf, (1, OH, 1), K, K, (1, H, 1), N, N, (1, KY, 1), (1, 1, 1), (0, 0, 0), groups=G,
                                   ldw=N if fwd_planes else K, flags=capi.F_NFAST | (capi.F_BKMAJOR if fwd_planes else 0))
    d["wgstride"] = K * KY * N
    return desc.trim_conv(d)


def _variant(d, ws_floats=0):
    return capi.variant("pc_conv_variant", C.byref(ops.conv_desc(dict(d, flags=d["flags"] | capi.F_X6))), ws_floats)


def _run_pair(G, nf, K, N, x, planes_f, planes_t, tile):
    """-> the flagged launch's outputs (on planes_f [3][G][K][KY][N]), without and with a tail-split workspace, after requiring each
    bit-equal to the unflagged launch on planes_t [3][G][N][KY][K]."""
    df, dt = _dgrad(G, nf, K, N, True), _dgrad(G, nf, K, N, False)
    n_ws = ops.conv_x6_ws_floats(dt)
    assert n_ws > 0 and ops.conv_x6_ws_floats(df) == n_ws
    for ws_floats in (0, n_ws):
        v = _variant(dt, ws_floats)
        assert v.startswith("x6:%s:" % tile) and _variant(df, ws_floats) == v, (v, _variant(df, ws_floats))
    assert ":ks1" in _variant(dt, 0) and ":ks1" not in _variant(dt, n_ws)
    outs = []
    for split in (False, True):
        ws_f = torch.zeros(n_ws, device=DEV) if split else None
        ws_t = torch.zeros(n_ws, device=DEV) if split else None
        got = ops.conv_fwd_x6(df, x, planes_f.view(3, -1), torch.full((G * nf, H, N), 7.0, device=DEV), ws=ws_f)
        ref = ops.conv_fwd_x6(dt, x, planes_t.view(3, -1), torch.full((G * nf, H, N), -7.0, device=DEV), ws=ws_t)
        assert torch.equal(got, ref), "%s: %d of %d elements differ, max |diff| %.3e" % (
            "tail split" if split else "one block per tile", (got != ref).sum().item(), got.numel(), (got - ref).abs().max().item())
        outs.append(got)          # (the K slices are added in slice order: the split sum need not be bit-equal to the unsplit one)
    return outs


@pytest.mark.gpu
def test_bkmajor_on_the_spectral_producers_planes():
    """The issue's case: 4 groups (one complex frequency = 3 planes, one real), 96 -> 160 channels, 2 samples per group; weights from
    pc_wspec_master_planes on a random 96 x 160 x 9 x 9 master with out_f and out_t both produced."""
    G, nf, K, N, U, Ur = 4, 2, 96, 160, 2, 1
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(K, N, KY, 9, generator=g) / 30).to(DEV)
    tw = torch.randn(U, 9, 2, generator=g).to(DEV)
    nW = G * K * KY * N
    pf = torch.empty(3, nW, device=DEV, dtype=torch.int16)
    pt = torch.empty(3, nW, device=DEV, dtype=torch.int16)
    capi.call("pc_wspec_master_planes", ops.ptr(w), ops.ptr(tw), K, 0, K, N, KY, 9, U, Ur, ops.ptr(pf), ops.ptr(pt), nW, ops.stream())
    # the two layouts hold the same values: out_t is the transpose of out_f
    assert torch.equal(pf.view(3, G, K, KY, N).permute(0, 1, 4, 3, 2), pt.view(3, G, N, KY, K))
    x = torch.randn(G * nf, OH, K, generator=g).to(DEV)
    for out in _run_pair(G, nf, K, N, x, pf, pt, "64x64"):
        assert torch.isfinite(out).all() and out.abs().max().item() > 0


# (groups, samples per group, N): the smallest launches that take the 64 x 128 tile (164 blocks fill one round where the 64-column tiles
# would need two) and the 128 x 64 tile (same, against 64-row tiles); N has a ragged last column tile in both
TILE_CASES = [(41, 2, 416, "64x128"), (41, 4, 224, "128x64")]


@pytest.mark.gpu
@pytest.mark.parametrize("G,nf,N,tile", TILE_CASES)
def test_bkmajor_tiles_of_the_primary_caps_dgrad(G, nf, N, tile):
    K = 96
    g = torch.Generator().manual_seed(6)
    # random bf16 terms of decreasing magnitude, as pc_split_planes leaves them
    vals = torch.randn(3, G, K, KY, N, generator=g) * torch.tensor([1.0, 2.0 ** -9, 2.0 ** -18]).view(3, 1, 1, 1, 1) / 30
    pf = vals.to(torch.bfloat16).view(torch.int16).to(DEV)
    pt = pf.permute(0, 1, 4, 3, 2).contiguous()
    x = torch.randn(G * nf, OH, K, generator=g).to(DEV)
    _run_pair(G, nf, K, N, x, pf, pt, tile)


@pytest.mark.gpu
@pytest.mark.parametrize("G,nf,N,tile", [(4, 2, 160, "64x64")] + TILE_CASES)
def test_bkmajor_small_integers_are_exact(G, nf, N, tile):
    """Integer operands in [-3, 3] (one bf16 term each, the other planes zero): every product and every partial sum is an integer below
    2^24, so fp32 accumulation is exact in any order and the result must EQUAL the float64 sum.  Every (k, n) weight is distinct enough
    that pairing element e of the A fragment with another k of the B fragment changes the sum."""
    K = 96
    g = torch.Generator().manual_seed(7)
    wi = torch.randint(-3, 4, (G, K, KY, N), generator=g).float()
    pf = torch.zeros(3, G, K, KY, N, dtype=torch.int16)
    pf[0] = wi.to(torch.bfloat16).view(torch.int16)
    pf = pf.to(DEV)
    pt = pf.permute(0, 1, 4, 3, 2).contiguous()
    xi = torch.randint(-3, 4, (G, nf, OH, K), generator=g).float()
    outs = _run_pair(G, nf, K, N, xi.view(G * nf, OH, K).to(DEV), pf, pt, tile)
    ref = torch.zeros(G, nf, H, N, dtype=torch.float64)
    for k in range(KY):                                       # big[o] += small[i] w[k], o = i + k (desc.transposed_classes)
        ref[:, :, k:k + OH] += torch.einsum("gnic,gcd->gnid", xi.double(), wi[:, :, k].double())
    for out in outs:
        assert torch.equal(out.cpu().double().view(G, nf, H, N), ref)


def test_bkmajor_refuses_a_tile_it_is_not_built_for():
    """Host only (no GPU call is reached): 32 output channels take the 128 x 32 tile, for which the K-major fetch is not instantiated --
    the launch and its variant reporter return the argument error instead of running another kernel."""
    (d,) = desc.transposed_classes(8, (1, OH, 1), 96, 96, (1, H, 1), 32, 32, (1, KY, 1), (1, 1, 1), (0, 0, 0), groups=4, ldw=32,
                                   flags=capi.F_NFAST | capi.F_BKMAJOR | capi.F_X6)
    d["wgstride"] = 96 * KY * 32
    cd = ops.conv_desc(desc.trim_conv(d))
    lib = capi.lib()
    buf = C.create_string_buffer(160)
    assert lib.pc_conv_variant(C.byref(cd), 0, buf, 160) == -1 and b"PC_F_BKMAJOR" in lib.pc_last_error()
    fake = C.c_void_p(4096)                                    # aligned, never dereferenced: the descriptor is refused before any launch
    assert lib.pc_conv_fwd_x6(C.byref(cd), fake, fake, 4 * 96 * KY * 32, None, None, fake, None, None) == -1
    assert b"128 x 32" in lib.pc_last_error()
    # the same descriptor without the flag is a launch the library takes (its variant is reported) ...
    cd.flags &= ~capi.F_BKMAJOR
    cd.ldw = 96
    assert lib.pc_conv_variant(C.byref(cd), 0, buf, 160) == 0 and buf.value.startswith(b"x6:128x32:")
    # ... and the flag with output channels that are no multiple of 8 is refused whatever the tile
    (e,) = desc.transposed_classes(8, (1, OH, 1), 96, 96, (1, H, 1), 164, 164, (1, KY, 1), (1, 1, 1), (0, 0, 0), groups=4, ldw=168,
                                   flags=capi.F_NFAST | capi.F_BKMAJOR | capi.F_X6)
    assert lib.pc_conv_variant(C.byref(ops.conv_desc(desc.trim_conv(e))), 0, buf, 160) == -1 and b"Co % 8" in lib.pc_last_error()
