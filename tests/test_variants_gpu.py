"""GPU: every kernel-variant class of the training step (tests/variant_cases.py: one launch per class, at the real layer shape of the smallest
step size that selects it) against a float64 reference, through the C-ABI.

Reference: torch conv3d / autograd in float64 on the CPU, built from the descriptor alone (stride = istr, dilation = istep, padding from
ioff0, the weight taps wk0 + a * wkstep gathered from the full kernel, the output lattice scattered at q * ostr + ooff), the epilogue (bias,
activation from a channel on, Dropout3d scale, accumulate) applied in float64.  Operands as the step has them: forward launches read ReLU
outputs with per-channel scales, backward launches gradients of mixed sign; weight gradients multiply one of each.

Bars, all taken from the existing kernel tests:
  fp32 MFMA kernels     max |err| <= 2e-4 of the reference's scale            (close() of tests/test_kernels_gpu.py)
  Winograd              max |err| <= 2e-5 * max(1, scale)                      (tests/test_wino_gpu.py, tests/test_wino4_gpu.py)
  bf16-split kernels    e <= 1.05 * e_native + 1e-9 and e < 2e-6 (conv) / 5e-6 (weight gradient), e = sum |err| / sum |ref|
                        (tests/test_x6_gpu.py) -- where the native launch of the same descriptor has itself passed the fp32 bar
  channel slices        the buffer outside [c0, c0 + C) keeps its sentinel bit for bit
  BatchNorm partials    per batch group, summed in float64, against the float64 column sums of the reference: 2e-4 of their scale
  tail-split launches   workspace zeroed once, two runs bit-identical, counters back at zero
Before launching, each case asserts that the library reports the class it is filed under.  Every case appends (e_hip, the float32 CPU
result's own distance from float64) to test_records/variants.json -- records, not bars (docs/NUMERICS.md has the table)."""
import json
import os
import re
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from picons_amd import capi, desc as D, ops
from tests import variant_cases as V
from tests.test_kernels_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.25
RECORDS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_records", "variants.json")
_T0 = time.time()


def _rel(a, ref):
    return ((a.double() - ref).abs().sum() / ref.abs().sum()).item()


def _record(case, **kw):
    os.makedirs(os.path.dirname(RECORDS), exist_ok=True)
    rows = {}
    if os.path.exists(RECORDS):
        try:
            rows = json.load(open(RECORDS))
        except ValueError:
            rows = {}
    rows[case["name"]] = dict(cls=repr(tuple(case["cls"])), sizes=case["sizes"], module_seconds=round(time.time() - _T0, 1), **kw)
    json.dump(rows, open(RECORDS, "w"), indent=1, sort_keys=True)


def _operand(g, shape, relu):
    """[..., C] operand: per-channel scales exp(N(0, 1)); relu: a ReLU output (half exact zeros), else a gradient of mixed sign."""
    x = torch.randn(*shape, generator=g) * torch.exp(torch.randn(shape[-1], generator=g))
    return torch.relu(x) if relu else x


def _c0(ld, C_):
    """Channel offset of a slice of C_ channels in rows of ld: as far right as 16-byte alignment allows."""
    return (ld - C_) // 4 * 4


# ------------------------------------------------------------------------------------------------------------------ references
def conv_reference(d, x, w, bias, cscale, base, dtype=torch.float64):
    """x [N][Ti][Hi][Wi][Ci], w [G][Co][KT*KH*KW][Ci] (G = groups with per-group weights, else 1), bias [G][Co] | None, cscale [N][Co] | None,
    base [N][To][Ho][Wo][Co] (what the output buffer holds before the launch) -> (out [N][To][Ho][Wo][Co], pre-epilogue lattice values
    [N][Co][Tq][Hq][Wq]), both in `dtype`."""
    N, Ci, Co = d["N"], d["Ci"], d["Co"]
    G = w.shape[0]
    I, Q, O = (d["Ti"], d["Hi"], d["Wi"]), (d["Tq"], d["Hq"], d["Wq"]), (d["To"], d["Ho"], d["Wo"])
    wk = w.to(dtype).view(G, Co, d["KT"], d["KH"], d["KW"], Ci)
    # tap a of a dimension reads position q * istr + ioff0 + a * istep with weight tap wk0 + a * wkstep; a mirrored gather (istep < 0: the input
    # gradients, the transposed convolutions) is the same sum with the taps walked from the other end
    idx, ioff, istep = [], [], []
    for i in range(3):
        taps = [d["wk0"][i] + a * d["wkstep"][i] for a in range(d["ntap"][i])]
        back = d["istep"][i] < 0
        idx.append(torch.tensor(taps[::-1] if back else taps))
        ioff.append(d["ioff0"][i] + (d["ntap"][i] - 1) * d["istep"][i] if back else d["ioff0"][i])
        istep.append(max(1, abs(d["istep"][i])))
    wk = wk.index_select(2, idx[0]).index_select(3, idx[1]).index_select(4, idx[2]).permute(0, 1, 5, 2, 3, 4).contiguous()
    pad = []
    for i in (2, 1, 0):
        left = -ioff[i]
        need = (Q[i] - 1) * d["istr"][i] + (d["ntap"][i] - 1) * istep[i] + 1
        pad += [left, need - (I[i] + left)]
    xp = F.pad(x.to(dtype).permute(0, 4, 1, 2, 3), pad)
    ng = N // G
    y = torch.cat([F.conv3d(xp[g * ng:(g + 1) * ng], wk[g], None, stride=[max(1, v) for v in d["istr"]], dilation=istep) for g in range(G)])
    assert tuple(y.shape[2:]) == Q, (y.shape, Q)
    v = y
    if d["flags"] & capi.F_BIAS:
        v = v + bias.to(dtype).repeat_interleave(N // bias.shape[0], 0).view(N, Co, 1, 1, 1)
    c0 = d["act_c0"]
    if d["act"] == capi.ACT_RELU:
        v = torch.cat([v[:, :c0], v[:, c0:].clamp_min(0)], 1)
    elif d["act"] == capi.ACT_SIGMOID:
        v = torch.cat([v[:, :c0], torch.sigmoid(v[:, c0:])], 1)
    if d["flags"] & capi.F_CSCALE:
        v = v * cscale.to(dtype).view(N, Co, 1, 1, 1)
    out = base.to(dtype).clone()
    sel = []
    for i in range(3):
        o = [q * d["ostr"][i] + d["ooff"][i] for q in range(Q[i])]
        assert all(0 <= a < O[i] for a in o), "lattice leaves the output"
        sel.append(torch.tensor(o))
    v = v.permute(0, 2, 3, 4, 1)
    it, ih, iw = torch.meshgrid(*sel, indexing="ij")
    if d["flags"] & capi.F_ACCUM:
        out[:, it, ih, iw] += v
    else:
        out[:, it, ih, iw] = v
    return out, y, (it, ih, iw)


def wino_reference(st, x, w, bias, base, dtype=torch.float64):
    """x [N][Ti][H][W][Ci], w [Co][Ci][KT][3][3] -> (out [N][T][H][W][Co], pre-epilogue values in the same layout)"""
    xin = x.to(dtype).permute(0, 4, 1, 2, 3)
    y = torch.zeros(st.N, st.Co, st.T, st.H, st.W, dtype=dtype)
    for t in range(st.T):
        for a in range(st.KT):
            num = t * st.ta + a + st.tc
            if num >= 0 and num % st.tden == 0 and num // st.tden < st.Ti:
                f = num // st.tden
                y[:, :, t] += F.conv3d(xin[:, :, f:f + 1], w.to(dtype)[:, :, a:a + 1], None, padding=(0, 1, 1))[:, :, 0]
    v = y
    if st.flags & capi.F_BIAS:
        v = v + bias.to(dtype).view(1, -1, 1, 1, 1)
    if st.act == capi.ACT_RELU:
        v = v.clamp_min(0)
    v = v.permute(0, 2, 3, 4, 1)
    return (base.to(dtype) + v if st.flags & capi.F_ACCUM else v.contiguous()), y.permute(0, 2, 3, 4, 1)


def wgrad_reference(d, Dl, S, dtype=torch.float64):
    """One problem: Dl [N][Tq][Hq][Wq][Cd] (the lattice values), S [N][Ts][Hs][Ws][Cs] -> g [Cd][KT*KH*KW][Cs] (taps the descriptor trimmed: 0)"""
    Q, I = (d["Tq"], d["Hq"], d["Wq"]), (d["Ts"], d["Hs"], d["Ws"])
    assert min(d["istep"]) >= 0, "mirrored weight-gradient gathers do not occur"
    pad = []
    for i in (2, 1, 0):
        left = -d["ioff0"][i]
        need = (Q[i] - 1) * d["istr"][i] + (d["ntap"][i] - 1) * d["istep"][i] + 1
        pad += [left, need - (I[i] + left)]
    xp = F.pad(S.to(dtype).permute(0, 4, 1, 2, 3), pad)
    W = torch.zeros(d["Cd"], d["Cs"], *d["ntap"], dtype=dtype, requires_grad=True)
    y = F.conv3d(xp, W, None, stride=[max(1, v) for v in d["istr"]], dilation=[max(1, v) for v in d["istep"]])
    assert tuple(y.shape[2:]) == Q
    y.backward(Dl.to(dtype).permute(0, 4, 1, 2, 3))
    g = torch.zeros(d["Cd"], d["KT"], d["KH"], d["KW"], d["Cs"], dtype=dtype)
    k0 = d["wk0"]
    g[:, k0[0]:k0[0] + d["ntap"][0], k0[1]:k0[1] + d["ntap"][1], k0[2]:k0[2] + d["ntap"][2]] = W.grad.permute(0, 2, 3, 4, 1)
    return g.view(d["Cd"], -1, d["Cs"])


# ------------------------------------------------------------------------------------------------------------------ runners
def _bn_check(part, groups, y, what):
    """part [rows][2][Co] (rows of a batch group contiguous), y: pre-epilogue reference [N][...][Co] channels-last, float64"""
    rows, Co = part.shape[0], part.shape[2]
    assert rows % groups == 0
    per, ng = rows // groups, y.shape[0] // groups
    p = part.cpu().double()
    for gi in range(groups):
        o = y[gi * ng:(gi + 1) * ng].reshape(-1, Co)
        s1, s2 = p[gi * per:(gi + 1) * per, 0].sum(0), p[gi * per:(gi + 1) * per, 1].sum(0)
        e1 = (s1 - o.sum(0)).abs().max().item() / o.abs().sum(0).max().item()
        e2 = (s2 - (o * o).sum(0)).abs().max().item() / (o * o).sum(0).max().item()
        print("%s: BatchNorm partials of group %d: sum %.3e, sum of squares %.3e of their scale" % (what, gi, e1, e2))
        assert e1 <= 2e-4 and e2 <= 2e-4, (what, gi, e1, e2)


def _run_conv(case):
    d = D.unflatten_conv(case["desc"])
    fl = d["flags"]
    x6 = bool(fl & capi.F_X6)
    g = torch.Generator().manual_seed(101)
    N, Ci, Co, ldi, ldo, ldw = d["N"], d["Ci"], d["Co"], d["ldi"], d["ldo"], d["ldw"]
    G = d["groups"] if d["wgstride"] else 1
    taps = d["KT"] * d["KH"] * d["KW"]
    P3 = d["To"] * d["Ho"] * d["Wo"]
    x = _operand(g, (N, d["Ti"], d["Hi"], d["Wi"], Ci), relu=case["list"] == "fwd")
    ci_real = 3 if fl & capi.F_CI3 else Ci
    K = ci_real * d["ntap"][0] * d["ntap"][1] * d["ntap"][2]
    w = torch.randn(G, Co, taps, Ci, generator=g) / np.sqrt(K)
    bias = torch.randn(G if d["bgstride"] else 1, Co, generator=g) if fl & capi.F_BIAS else None
    cscale = (torch.rand(N, Co, generator=g) < 0.5).float() * 2 if fl & capi.F_CSCALE else None
    accum = bool(fl & capi.F_ACCUM)
    base = torch.randn(N, d["To"], d["Ho"], d["Wo"], Co, generator=g) if accum else torch.full((N, d["To"], d["Ho"], d["Wo"], Co), SENTINEL)
    xr = x.clone()
    if fl & capi.F_CI3:
        xr[..., 3] = 0                                     # "taken as zero whatever it holds"
    ref_full, y64, lat = conv_reference(d, xr, w, bias, cscale, base)
    ref32, _, _ = conv_reference(d, xr, w, bias, cscale, base, torch.float32)
    # the error figures are taken over the positions the launch writes (a parity class of a transposed convolution writes one in eight);
    # every other position of the slice must keep what it held
    ref, ref32 = ref_full[:, lat[0], lat[1], lat[2]], ref32[:, lat[0], lat[1], lat[2]]
    off = torch.ones(d["To"], d["Ho"], d["Wo"], dtype=torch.bool)
    off[lat[0], lat[1], lat[2]] = False
    # device operands in the buffers the descriptor describes
    ci0, co0 = _c0(ldi, Ci), _c0(ldo, Co)
    xb = torch.full((N, d["Ti"], d["Hi"], d["Wi"], ldi), SENTINEL)
    xb[..., ci0:ci0 + Ci] = x
    xb = xb.to(DEV)
    wn = Co * taps * ldw
    assert d["wgstride"] == 0 or d["wgstride"] >= wn
    wb = torch.zeros((G - 1) * d["wgstride"] + wn)           # group g's weights at + g * wgstride floats
    for gi in range(G):
        wb[gi * d["wgstride"]:gi * d["wgstride"] + wn].view(Co, taps, ldw)[..., :Ci] = w[gi]
    wb = wb.to(DEV)
    if bias is not None and bias.shape[0] > 1:
        assert d["bgstride"] >= Co
        bb = torch.zeros((G - 1) * d["bgstride"] + Co)
        for gi in range(G):
            bb[gi * d["bgstride"]:gi * d["bgstride"] + Co] = bias[gi]
    elif bias is not None:
        bb = bias[0].clone()
    tout = bool(fl & capi.F_TOUT)

    def out_buffer():
        if tout:
            ob = torch.full((N, ldo, P3), SENTINEL)
            ob[:, co0:co0 + Co] = base.view(N, P3, Co).permute(0, 2, 1)
        else:
            ob = torch.full((N, d["To"], d["Ho"], d["Wo"], ldo), SENTINEL)
            ob[..., co0:co0 + Co] = base
        return ob.to(DEV)

    def launch(dd, split, ws=None):
        ob = out_buffer()
        ov = ob[:, co0:] if tout else ob[..., co0:]
        part = torch.zeros(ops.conv_bnpart_rows(dd), 2, Co, device=DEV) if fl & capi.F_BNPART else None
        bd, cd = (bb.to(DEV) if bias is not None else None), (cscale.to(DEV) if cscale is not None else None)
        if split:
            ops.conv_fwd_x6(dd, xb[..., ci0:], ops.split_planes(wb), ov, bias=bd, cscale=cd, bnpart=part, ws=ws)
        else:
            ops.conv_fwd(dd, xb[..., ci0:], wb, ov, bias=bd, cscale=cd, bnpart=part)
        torch.cuda.synchronize()
        o = ob.cpu()
        if tout:
            got = o[:, co0:co0 + Co].permute(0, 2, 1).reshape(N, d["To"], d["Ho"], d["Wo"], Co).clone()
            o[:, co0:co0 + Co] = SENTINEL
        else:
            got = o[..., co0:co0 + Co].clone()
            o[..., co0:co0 + Co] = SENTINEL
        assert torch.equal(o, torch.full_like(o, SENTINEL)), "the launch wrote outside its channel slice"
        assert torch.equal(got[:, off], base[:, off]), "the launch wrote outside its output lattice"
        return got[:, lat[0], lat[1], lat[2]], part

    what = V.case_id(case)
    nat_d = dict(d, flags=fl & ~capi.F_X6)
    nat, part = launch(nat_d, False)
    e_nat, e_32 = _rel(nat, ref), _rel(ref32, ref)
    print("%s: fp32 MFMA e = %.3e, max %.3e of scale %.3e; float32 CPU e = %.3e" % (what, e_nat, (nat.double() - ref).abs().max().item(), ref.abs().max().item(), e_32))
    close(nat, ref, what=what + " (fp32 MFMA kernel)")
    if part is not None:
        _bn_check(part, d["groups"], y64.permute(0, 2, 3, 4, 1), what)
    if not x6:
        _record(case, e_hip=e_nat, e_f32_cpu=e_32)
        return
    ks = int(re.search(r":ks(\d+)", case["cls"][1]).group(1))
    ws = torch.zeros(case["ws"], device=DEV) if ks > 1 else None
    assert (ks > 1) == (case["ws"] > 0)
    got, part = launch(d, True, ws)
    e_x6 = _rel(got, ref)
    print("%s: bf16-split e = %.3e against native %.3e" % (what, e_x6, e_nat))
    close(got, ref, what=what + " (bf16-split kernel)")
    if part is not None:
        _bn_check(part, d["groups"], y64.permute(0, 2, 3, 4, 1), what)
    if ks > 1:
        bm, bn = [int(v) for v in re.match(r"x6:(\d+)x(\d+):", case["cls"][1]).groups()]
        rem = case["ws"] // (ks * bm * bn)
        ctr = ws[rem * ks * bm * bn:].view(torch.int32)
        assert ctr.numel() == (rem + 3) // 4 * 4 and int(ctr.abs().sum()) == 0, "tile counters not back at zero"
        again, _ = launch(d, True, ws)
        assert torch.equal(again, got), "tail-split launch not bit-identical from run to run"
        assert int(ctr.abs().sum()) == 0
    _record(case, e_hip=e_x6, e_native=e_nat, e_f32_cpu=e_32)
    assert e_x6 <= 1.05 * e_nat + 1e-9, "%s: bf16-split error %.3e vs native fp32 MFMA %.3e (against fp64)" % (what, e_x6, e_nat)
    assert e_x6 < 2e-6


def _run_wino(case):
    import ctypes as C
    st = V.wino_struct(case["desc"])
    g = torch.Generator().manual_seed(103)
    N, Ci, Co, ldi, ldo = st.N, st.Ci, st.Co, st.ldi, st.ldo
    x = _operand(g, (N, st.Ti, st.H, st.W, Ci), relu=case["list"] == "fwd")
    w = torch.randn(Co, Ci, st.KT, 3, 3, generator=g) / np.sqrt(Ci * st.KT * 9)
    bias = torch.randn(Co, generator=g) if st.flags & capi.F_BIAS else None
    accum = bool(st.flags & capi.F_ACCUM)
    base = torch.randn(N, st.T, st.H, st.W, Co, generator=g) if accum else torch.full((N, st.T, st.H, st.W, Co), SENTINEL)
    ref, y64 = wino_reference(st, x, w, bias, base)
    ref32, _ = wino_reference(st, x, w, bias, base, torch.float32)
    ci0, co0 = _c0(ldi, Ci), _c0(ldo, Co)
    xb = torch.full((N, st.Ti, st.H, st.W, ldi), SENTINEL)
    xb[..., ci0:ci0 + Ci] = x
    ob = torch.full((N, st.T, st.H, st.W, ldo), SENTINEL)
    ob[..., co0:co0 + Co] = base
    xb, ob = xb.to(DEV), ob.to(DEV)
    m = 4 if st.m == 4 else 2
    U = ops.wino_weights(w.to(DEV).contiguous(), Co, Ci, st.KT, m=m)
    part = torch.zeros(capi.lib().pc_wino_bnpart_rows(C.byref(st)), 2, Co, device=DEV) if st.flags & capi.F_BNPART else None
    ops.wino_conv(st, xb[..., ci0:], U, ob[..., co0:], bias=bias.to(DEV) if bias is not None else None, bnpart=part)
    torch.cuda.synchronize()
    o = ob.cpu()
    got = o[..., co0:co0 + Co].clone()
    o[..., co0:co0 + Co] = SENTINEL
    assert torch.equal(o, torch.full_like(o, SENTINEL)), "the launch wrote outside its channel slice"
    what = V.case_id(case)
    err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    e, e_32 = _rel(got, ref), _rel(ref32, ref)
    print("%s: Winograd max err %.3e at scale %.3e (bar %.3e), e = %.3e; float32 CPU e = %.3e" % (what, err, scale, 2e-5 * max(1.0, scale), e, e_32))
    _record(case, e_hip=e, e_f32_cpu=e_32, max_err_over_scale=err / max(1.0, scale))
    assert err <= 2e-5 * max(1.0, scale), (what, err, scale)
    if part is not None:
        _bn_check(part, 2, y64, what)


def _run_wgrad(case):
    d = V.unflatten_wgrad(case["desc"])
    g = torch.Generator().manual_seed(107)
    nb = max(1, d["nbatch"])
    N, Cd, Cs, ldd, lds = d["N"], d["Cd"], d["Cs"], d["ldd"], d["lds"]
    taps = d["KT"] * d["KH"] * d["KW"]
    dlat = d["Td"] > 0
    dshape = (N, d["Td"], d["Hd"], d["Wd"], ldd) if dlat else (N, d["Tq"], d["Hq"], d["Wq"], ldd)
    sshape = (N, d["Ts"], d["Hs"], d["Ws"], lds)
    dn, sn = int(np.prod(dshape)), int(np.prod(sshape))
    dbs, sbs, gbs = (d["dbstride"], d["sbstride"], d["gbstride"]) if nb > 1 else (dn, sn, Cd * taps * Cs)
    cd0, cs0 = _c0(ldd, Cd), _c0(lds, Cs)
    Db = torch.full(((nb - 1) * dbs + dn + cd0,), SENTINEL)
    Sb = torch.full(((nb - 1) * sbs + sn + cs0,), SENTINEL)
    refs, refs32 = [], []
    cs_real = 3 if d["flags"] & capi.WG_CS3 else Cs
    for b in range(nb):
        Dt = _operand(g, dshape[:4] + (Cd,), relu=False)
        St = _operand(g, sshape[:4] + (Cs,), relu=True)
        St[..., cs_real:] = 0
        Db[cd0 + b * dbs:cd0 + b * dbs + dn].view(dshape)[..., :Cd] = Dt
        Sb[cs0 + b * sbs:cs0 + b * sbs + sn].view(sshape)[..., :Cs] = St
        o = d["doff"]
        Dl = Dt[:, o[0]:o[0] + d["Tq"], o[1]:o[1] + d["Hq"], o[2]:o[2] + d["Wq"]] if dlat else Dt
        refs.append(wgrad_reference(d, Dl, St))
        refs32.append(wgrad_reference(d, Dl, St, torch.float32))
    ref, ref32 = torch.stack(refs)[..., :cs_real], torch.stack(refs32)[..., :cs_real]
    Dd, Sd = Db.to(DEV), Sb.to(DEV)
    image = gbs * nb if nb > 1 else Cd * taps * Cs

    def launch(dd):
        if dd["splitk"] == -1:
            buf = torch.full((image,), SENTINEL, device=DEV)             # plain stores: g need not be initialised
            ops.conv_wgrad(dict(dd, ws_slices=0), Dd[cd0:], Sd[cs0:], buf)
            tot = buf
        else:
            ns = dd["ws_slices"] if dd["ws_slices"] > 0 else ops.wgrad_slices(dd)
            buf = torch.zeros(ns, image, device=DEV)
            ops.conv_wgrad(dict(dd, ws_slices=ns), Dd[cd0:], Sd[cs0:], buf)
            tot = buf[0].clone()
            for k in range(1, ns):
                tot += buf[k]
        torch.cuda.synchronize()
        t = tot.cpu()
        return torch.stack([t[b * gbs:b * gbs + Cd * taps * Cs].view(Cd, taps, Cs) for b in range(nb)])[..., :cs_real]

    what = V.case_id(case)
    x6 = bool(capi.lib().pc_wgrad_uses_x6(ops._fill_struct(capi.WgradDesc(), d)))
    nat = launch(dict(d, flags=d["flags"] & ~capi.WG_X6, ws_slices=0))
    e_nat, e_32 = _rel(nat, ref), _rel(ref32, ref)
    print("%s: fp32 MFMA e = %.3e, max %.3e of scale %.3e; float32 CPU e = %.3e" % (what, e_nat, (nat.double() - ref).abs().max().item(), ref.abs().max().item(), e_32))
    close(nat, ref, what=what + " (fp32 MFMA kernel)")
    if not x6:
        _record(case, e_hip=e_nat, e_f32_cpu=e_32)
        return
    got = launch(d)
    e_x6 = _rel(got, ref)
    print("%s: bf16-split e = %.3e against native %.3e" % (what, e_x6, e_nat))
    close(got, ref, what=what + " (bf16-split kernel)")
    _record(case, e_hip=e_x6, e_native=e_nat, e_f32_cpu=e_32)
    assert e_x6 <= 1.05 * e_nat + 1e-9, "%s: bf16-split error %.3e vs native fp32 MFMA %.3e (against fp64)" % (what, e_x6, e_nat)
    assert e_x6 < 5e-6


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_variant_class_vs_fp64(case):
    t0 = time.time()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    got = V.case_class(case)
    assert got == tuple(case["cls"]), "%s: filed under %r, the library reports %r" % (case["name"], case["cls"], got)
    {"conv": _run_conv, "wino": _run_wino, "wgrad": _run_wgrad}[case["kind"]](case)
    print("%s: %.1f s (module so far %.1f s)" % (V.case_id(case), time.time() - t0, time.time() - _T0))


def test_records_hold_one_row_per_class():
    rows = json.load(open(RECORDS))
    assert sorted(rows) == sorted(c["name"] for c in V.CASES), set(rows) ^ {c["name"] for c in V.CASES}
    print("tests/test_variants_gpu.py: %d classes, module wall time %.1f s" % (len(rows), time.time() - _T0))
