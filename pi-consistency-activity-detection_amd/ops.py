"""Thin torch-tensor wrappers over the C-ABI (one per entry point).  PyTorch is used for device
memory and streams only; every wrapper launches HIP kernels from libpicons.so on torch's current
stream and raises if the tensor is not on a GPU - there is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import capi, desc as D


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("picons ops need CUDA/HIP tensors (no CPU fallback)")
    return C.c_void_p(t.data_ptr())


def _fill_struct(st, d):
    for name, ctype in st._fields_:
        v = d[name]
        if isinstance(v, (list, tuple)):
            setattr(st, name, (C.c_int32 * 3)(*[int(x) for x in v]))
        else:
            setattr(st, name, ctype(v))
    return st


def conv_desc(d):
    return _fill_struct(capi.ConvDesc(), d)


def conv_bnpart_rows(d):
    return capi.lib().pc_conv_bnpart_rows(C.byref(conv_desc(d)))


def conv_fwd(d, x, w, out, bias=None, cscale=None, bnpart=None):
    capi.call("pc_conv_fwd", C.byref(conv_desc(d)), ptr(x), ptr(w), ptr(bias), ptr(cscale), ptr(out), ptr(bnpart), stream())
    return out


def split_planes(w):
    """fp32 device tensor (numel % 4 == 0) -> int16 tensor [3][numel]: the bf16 terms h, m, l of every element (pc_split_planes)."""
    n = w.numel()
    planes = torch.empty(3, n, device=w.device, dtype=torch.int16)
    capi.call("pc_split_planes", ptr(w), ptr(planes), n, n, stream())
    return planes


def conv_x6_ws_floats(d):
    """Floats of workspace pc_conv_fwd_x6_ws would use to split the tiles of the launch's last round into K slices (0: it would not)."""
    dd = dict(d)
    dd["flags"] = int(dd.get("flags", 0)) | capi.F_X6
    return int(capi.lib().pc_conv_x6_ws_floats(C.byref(conv_desc(dd))))


def conv_fwd_x6(d, x, wplanes, out, bias=None, cscale=None, bnpart=None, ws=None):
    """pc_conv_fwd_x6: d as for conv_fwd (PC_F_X6 is added here), wplanes = split_planes(w) of the [Co][taps][ldw] weights.
    ws: a ZEROED float32 device tensor of conv_x6_ws_floats(d) elements (or more) lets the launch split its tail tiles along K."""
    dd = dict(d)
    dd["flags"] = int(dd.get("flags", 0)) | capi.F_X6
    if ws is None:
        capi.call("pc_conv_fwd_x6", C.byref(conv_desc(dd)), ptr(x), ptr(wplanes), wplanes.shape[1], ptr(bias), ptr(cscale), ptr(out), ptr(bnpart), stream())
    else:
        capi.call("pc_conv_fwd_x6_ws", C.byref(conv_desc(dd)), ptr(x), ptr(wplanes), wplanes.shape[1], ptr(bias), ptr(cscale), ptr(out), ptr(bnpart),
                  ptr(ws), ws.numel(), stream())
    return out


def wino_desc(N, T, H, W, Ci, ldi, Co, ldo, KT=3, act=0, flags=0, Ti=None, ta=1, tc=None, tden=1, m=2):
    """pc_wino_desc; defaults = temporal stride 1 with padding KT // 2 (see include/picons.h for (ta, tc, tden)); m = 2: F(2x2, 3x3),
    4: F(4x4, 3x3) (U from wino_weights(..., m=4))."""
    st = capi.WinoDesc()
    st.m = m
    st.N, st.T, st.H, st.W, st.Ci, st.ldi, st.Co, st.ldo, st.KT, st.act, st.flags = N, T, H, W, Ci, ldi, Co, ldo, KT, act, flags
    st.Ti, st.ta, st.tc, st.tden = (T if Ti is None else Ti), ta, (-(KT // 2) if tc is None else tc), tden
    return st


def wino_weights(w, O, I, KT=3, flip=False, strides=None, out=None, m=2):
    """Transform-domain weights of pc_wino_conv from a weight tensor addressed as w[o*sO + tap*sT + i*sI] (default: contiguous
    OIDHW, i.e. (O, I, KT, 3, 3))."""
    sO, sT, sI = strides if strides is not None else (I * KT * 9, 1, KT * 9)
    fam = "pc_wino4" if m == 4 else "pc_wino"
    n = getattr(capi.lib(), fam + "_u_floats")(O, I, KT)
    U = out if out is not None else torch.empty(n, device=w.device, dtype=torch.float32)
    capi.call(fam + "_weights", ptr(w), int(sO), int(sT), int(sI), O, I, KT, int(flip), ptr(U), stream())
    return U


def wino_weights_multi(jobs):
    """pc_wino_weights_multi: jobs = [(w, U, (sO, sT, sI), O, I, KT, flip, m)] with device tensors w, U -- every job in ONE launch."""
    tab = np.zeros(len(jobs), dtype=capi.WWJOB_DTYPE)
    for q, (w, U, st, O, I, KT, flip, m) in enumerate(jobs):
        tab[q] = (w.data_ptr(), U.data_ptr(), st[0], st[1], st[2], O, I, KT, int(flip), m, 0)
    capi.call("pc_wino_weights_multi", C.c_void_p(tab.ctypes.data), len(jobs), stream())


def wino_conv(d, x, U, out, bias=None, bnpart=None):
    capi.call("pc_wino_conv", C.byref(d), ptr(x), ptr(U), ptr(bias), ptr(out), ptr(bnpart), stream())
    return out


def conv_wgrad(d, Dt, St, g):
    capi.call("pc_conv_wgrad", C.byref(_fill_struct(capi.WgradDesc(), d)), ptr(Dt), ptr(St), ptr(g), stream())
    return g


def wgrad_slices(d):
    """K slices pc_conv_wgrad makes for descriptor d (host-only): the workspace images an ordered (atomic-free) launch needs."""
    n = capi.lib().pc_wgrad_slices(C.byref(_fill_struct(capi.WgradDesc(), dict(d, ws_slices=0))))
    if n < 1:
        raise RuntimeError("pc_wgrad_slices: %s" % capi.lib().pc_last_error().decode())
    return int(n)


def conv_wgrad_ordered(d, Dt, St, ws=None):
    """The weight gradient without atomics: the K slices leave their partial sums in `ws` ([slices][Cd][taps][Cs], zero before its first
    use) and are added in slice order -> (g [Cd][taps][Cs], ws).  Bit-identical from run to run."""
    n = wgrad_slices(d)
    taps = d["KT"] * d["KH"] * d["KW"]
    image = d["gbstride"] * d["nbatch"] if d.get("nbatch", 0) > 1 else d["Cd"] * taps * d["Cs"]
    if ws is None:
        ws = torch.zeros(n * image, device=Dt.device, dtype=torch.float32)
    conv_wgrad(dict(d, ws_slices=n), Dt, St, ws)
    g = ws.view(n, image)[0].clone()
    for k in range(1, n):
        g += ws.view(n, image)[k]
    return g, ws


def wgrad_fold(ws, image_floats, nslices):
    """pc_wgrad_fold: the K-slice images of `ws` folded in place to groups of pc_wgrad_fold_group() (slice order)."""
    capi.call("pc_wgrad_fold", ptr(ws), int(image_floats), int(nslices), stream())
    return ws


def wgrad_job_table(jobs):
    """[(desc dict, D ptr, S ptr, g ptr)] with integer device addresses -> host array of pc_wgrad_job."""
    tab = np.zeros(len(jobs), dtype=capi.WJOB_DTYPE)
    for q, (d, Dp, Sp, gp) in enumerate(jobs):
        tab[q]["d"][:] = D.flatten(d, D.WGRAD_FIELDS)
        tab[q]["D"], tab[q]["S"], tab[q]["g"] = Dp, Sp, gp
    return tab


def conv_wgrad_multi(jobs):
    """jobs: [(desc dict, D tensor, S tensor, g tensor)]: pc_conv_wgrad_multi (one grid for the generic split-K problems)."""
    tab = wgrad_job_table([(d, Dt.data_ptr(), St.data_ptr(), g.data_ptr()) for d, Dt, St, g in jobs])
    for _d, Dt, St, g in jobs:
        ptr(Dt); ptr(St); ptr(g)
    capi.call("pc_conv_wgrad_multi", C.c_void_p(tab.ctypes.data), len(jobs), stream())


def bn_finalize(part, npg, groups, C_, count, gamma, beta, eps, momentum, rmean=None, rvar=None, two_stage=False):
    """two_stage: with the workspace of pc_bn_finalize_ws (the plan's form; a no-op below 512 partial rows per group)."""
    stat = torch.empty(groups, 4, C_, device=part.device, dtype=torch.float32)
    if two_stage:
        n = capi.lib().pc_bn_finalize_ws_floats(npg, groups, C_)
        ws = torch.empty(max(int(n), 1), device=part.device, dtype=torch.float32)
        capi.call("pc_bn_finalize_ws", ptr(part), npg, groups, C_, int(count), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                  ptr(stat), ptr(ws) if n > 0 else None, stream())
    else:
        capi.call("pc_bn_finalize", ptr(part), npg, groups, C_, int(count), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar),
                  ptr(stat), stream())
    return stat


def bn_finalize_apply(part, npg, groups, C_, count, gamma, beta, eps, momentum, rmean, rvar, z, ldz, rows, y, ldy, relu=True):
    """pc_bn_finalize_apply: the statistics and the normalised output in one launch (npg <= 256 partial rows per group) -> stat."""
    stat = torch.empty(groups, 4, C_, device=part.device, dtype=torch.float32)
    capi.call("pc_bn_finalize_apply", ptr(part), npg, groups, C_, int(count), ptr(gamma), ptr(beta), eps, momentum, ptr(rmean), ptr(rvar), ptr(stat),
              ptr(z), ldz, int(rows), ptr(y), ldy, int(relu), stream())
    return stat


def bn_apply(z, ldz, stat, C_, rows, groups, y, ldy, relu=True):
    capi.call("pc_bn_apply", ptr(z), ldz, ptr(stat), C_, int(rows), groups, ptr(y), ldy, int(relu), stream())
    return y


def bn_eval_stat(gamma, beta, rm, rv, eps):
    stat = torch.empty(1, 4, gamma.numel(), device=gamma.device, dtype=torch.float32)
    capi.call("pc_bn_eval_stat", ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, gamma.numel(), ptr(stat), stream())
    return stat


def bn_bwd(dy, lddy, z, ldz, stat, C_, rows, groups, relu, dz, lddz, dgamma, dbeta, accum=False, fused=False):
    """fused: the finalize folded into the apply kernel (bit 1 of pc_bn_bwd's `relu`)."""
    ws = torch.empty(capi.lib().pc_bn_bwd_ws_floats(int(rows), C_, groups), device=dy.device, dtype=torch.float32)
    capi.call("pc_bn_bwd", ptr(dy), lddy, ptr(z), ldz, ptr(stat), C_, int(rows), groups, int(bool(relu)) | (2 if fused else 0), ptr(dz), lddz, ptr(dgamma), ptr(dbeta),
              int(accum), ptr(ws), stream())
    return dz


def maxpool_fwd(d, x, y, argmax):
    capi.call("pc_maxpool_fwd", C.byref(_fill_struct(capi.PoolDesc(), d)), ptr(x), ptr(y), ptr(argmax), stream())


def maxpool_bwd(d, dy, argmax, dx, accum=False):
    capi.call("pc_maxpool_bwd", C.byref(_fill_struct(capi.PoolDesc(), d)), ptr(dy), ptr(argmax), ptr(dx), int(accum), stream())


def channel_scale(x, ldx, scale, N, pos_per_n, C_, y, ldy, accum=False):
    capi.call("pc_channel_scale", ptr(x), ldx, ptr(scale), N, int(pos_per_n), C_, ptr(y), ldy, int(accum), stream())


def act_bwd(dy, lddy, y, ldy, act, C_, rows, dz, lddz, dbias=None, accum=False):
    ws = torch.empty(capi.lib().pc_act_bwd_ws_floats(int(rows), C_), device=dy.device, dtype=torch.float32)
    capi.call("pc_act_bwd", ptr(dy), lddy, ptr(y), ldy, act, C_, int(rows), ptr(dz), lddz, ptr(dbias), int(accum), ptr(ws), stream())


def to_ndhwc(src, Cpad=None, flipw=False):
    """src (N,C,T,H,W) fp32/fp64 contiguous -> (N,T,H,W,Cpad) fp32."""
    N, Cc, T, H, W = src.shape
    Cpad = Cpad or Cc
    dst = torch.empty(N, T, H, W, Cpad, device=src.device, dtype=torch.float32)
    capi.call("pc_ncdhw_to_ndhwc", ptr(src.contiguous()), int(src.dtype == torch.float64), N, Cc, T * H * W, W, Cpad, int(flipw), ptr(dst), stream())
    return dst


def to_ncdhw(src, C_=None):
    N, T, H, W, ld = src.shape
    C_ = C_ or ld
    dst = torch.empty(N, C_, T, H, W, device=src.device, dtype=torch.float32)
    capi.call("pc_ndhwc_to_ncdhw", ptr(src), ld, N, C_, T * H * W, ptr(dst), stream())
    return dst


def transpose_batched(src, batch, R, Cc, sbs, sld, dst, dbs, dld, accum=False):
    capi.call("pc_transpose_batched", ptr(src), batch, R, Cc, int(sbs), sld, ptr(dst), int(dbs), dld, int(accum), stream())


def em_fwd(x, W, bu, ba, npos, B, C_, state=None):
    """state: optional float32 device tensor of pc_em_state_floats(npos) floats the forward fills for em_bwd."""
    out = torch.empty(npos, C_ * 17, device=x.device, dtype=torch.float32)
    capi.call("pc_em_routing_fwd", ptr(x), ptr(W), ptr(bu), ptr(ba), npos, B, C_, ptr(out), ptr(state), stream())
    return out


def em_state(npos, device):
    return torch.empty(capi.lib().pc_em_state_floats(int(npos)), device=device, dtype=torch.float32)


def em_bwd(x, W, bu, ba, dout, npos, B, C_, dW, dbu, dba, state=None):
    dx = torch.empty(npos, B * 17, device=x.device, dtype=torch.float32)
    ws = torch.empty(capi.lib().pc_em_ws_floats(npos, B, C_), device=x.device, dtype=torch.float32)
    capi.call("pc_em_routing_bwd", ptr(x), ptr(W), ptr(bu), ptr(ba), ptr(dout), npos, B, C_, ptr(dx), ptr(dW), ptr(dbu), ptr(dba), ptr(ws), ptr(state), stream())
    return dx


def class_mask_fwd(caps, Bn, npos, C_, cls, labeled, mode):
    dev = caps.device
    pred = torch.empty(Bn, C_, device=dev); mask = torch.empty(Bn, C_, device=dev)
    masked = torch.empty(Bn, npos, C_ * 16, device=dev)
    capi.call("pc_class_mask_fwd", ptr(caps), Bn, npos, C_, ptr(cls), ptr(labeled), mode, ptr(pred), ptr(mask), ptr(masked), stream())
    return pred, mask, masked


def class_mask_bwd(dmasked, dpred, mask, Bn, npos, C_):
    dcaps = torch.empty(Bn, npos, C_ * 17, device=dmasked.device)
    capi.call("pc_class_mask_bwd", ptr(dmasked), ptr(dpred), ptr(mask), Bn, npos, C_, ptr(dcaps), stream())
    return dcaps


def tapsum_fwd(proj, bias):
    N, T, H, W, _ = proj.shape
    out = torch.empty(N, T, H, W, device=proj.device)
    capi.call("pc_tapsum_fwd", ptr(proj), N, T, H, W, ptr(bias), ptr(out), stream())
    return out


def tapsum_bwd(dout):
    N, T, H, W = dout.shape
    dproj = torch.empty(N, T, H, W, 32, device=dout.device)
    capi.call("pc_tapsum_bwd", ptr(dout), N, T, H, W, ptr(dproj), stream())
    return dproj


def loss_desc(B, T, H, W, bv=False, gv=False, n_frames=3, predict_maps=False, jhmdb=False, lower=None, upper=None,
              bv_wt=0.5, gv_wt=0.5, wt_loc=1.0, wt_cons=1.0, wt_ramp=0.0):
    d = capi.LossDesc()
    d.B, d.T, d.H, d.W = B, T, H, W
    d.bv, d.gv, d.n_frames, d.predict_maps, d.jhmdb = int(bv), int(gv), n_frames, int(predict_maps), int(jhmdb)
    d.lower_thresh = -1.0 if lower is None else lower
    d.upper_thresh = -1.0 if upper is None else upper
    d.bv_wt, d.gv_wt, d.wt_loc, d.wt_cons, d.wt_ramp = bv_wt, gv_wt, wt_loc, wt_cons, wt_ramp
    return d


def consistency_loss(d, output, flip_op, seg, labeled, want_masks=False):
    """output, flip_op, seg: (B,1,8,H,W) fp32 contiguous; labeled int32 (B,).  Returns
    (scalars[8], d_output, d_flip_op, mask_bv, mask_gv)."""
    dev = output.device
    scal = torch.zeros(8, device=dev)
    dO = torch.empty_like(output); dF = torch.empty_like(flip_op)
    mb = torch.zeros_like(output) if want_masks else None
    mg = torch.zeros_like(output) if want_masks else None
    ws = torch.empty(capi.lib().pc_loss_ws_floats(C.byref(d)), device=dev, dtype=torch.float32)
    capi.call("pc_consistency_loss", C.byref(d), ptr(output), ptr(flip_op), ptr(seg), ptr(labeled), ptr(scal), ptr(dO), ptr(dF),
              ptr(mb), ptr(mg), ptr(ws), stream())
    return scal, dO, dF, mb, mg


def var_mask(pred, flip_pred, n_frames=5, use_sig=False):
    B, _, T, H, W = pred.shape
    d = loss_desc(B, T, H, W)
    ws = torch.empty(capi.lib().pc_loss_ws_floats(C.byref(d)), device=pred.device, dtype=torch.float32)
    m = torch.empty(B, 1, T, H, W, device=pred.device)
    capi.call("pc_var_mask", ptr(pred.contiguous()), ptr(flip_pred.contiguous()), B, T, H, W, n_frames, int(use_sig), ptr(m), ptr(ws), stream())
    return m


def grad_mask(pred, lower=None, upper=None):
    B, _, T, H, W = pred.shape
    d = loss_desc(B, T, H, W)
    ws = torch.empty(capi.lib().pc_loss_ws_floats(C.byref(d)), device=pred.device, dtype=torch.float32)
    m = torch.empty(B, T, H, W, device=pred.device)
    capi.call("pc_grad_mask", ptr(pred.contiguous()), B, T, H, W, -1.0 if lower is None else lower, -1.0 if upper is None else upper,
              ptr(m), ptr(ws), stream())
    return m


def spread_loss(x, cls, labeled, m=0.2, wt=1.0, dx=None):
    out = torch.empty(2, device=x.device)
    capi.call("pc_spread_loss", ptr(x), ptr(cls), ptr(labeled), x.shape[0], x.shape[1], m, wt, ptr(out), ptr(dx), stream())
    return out


def adam_step(p, g, m, v, lr, step, b1=0.9, b2=0.999, eps=1e-6, gscale=1.0):
    capi.call("pc_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, b1, b2, eps, step, gscale, stream())


def axis_linear(d, x, M, out, bias=None):
    """d: dict with capi.AXIS_FIELDS (see include/picons.h pc_axis_desc)."""
    st = capi.AxisDesc(*[int(d[k]) for k in capi.AXIS_FIELDS])
    capi.call("pc_axis_linear", C.byref(st), ptr(x), ptr(M), ptr(bias), ptr(out), stream())
    return out


def wspec_fwd(w, tw, A, B, KY, KX, U, Ur, out):
    capi.call("pc_wspec_fwd", ptr(w), ptr(tw), A, B, KY, KX, U, Ur, ptr(out), stream())
    return out


def wspec_bwd(dV, tw, A, B, KY, KX, U, Ur, kg):
    capi.call("pc_wspec_bwd", ptr(dV), ptr(tw), A, B, KY, KX, U, Ur, ptr(kg), stream())
    return kg


def wspec_master_fwd(w, tw, Acnt, a0, Atot, B, KY, KX, U, Ur, out_f, out_t):
    capi.call("pc_wspec_master_fwd", ptr(w), ptr(tw), Acnt, a0, Atot, B, KY, KX, U, Ur, ptr(out_f), ptr(out_t), stream())


def wspec_master_bwd(dV, tw, Acnt, a0, Atot, B, KY, KX, U, Ur, dw, accum=False):
    capi.call("pc_wspec_master_bwd", ptr(dV), ptr(tw), Acnt, a0, Atot, B, KY, KX, U, Ur, ptr(dw), int(accum), stream())
    return dw


def tail6_weights(wf, N, Ci, W6f, W6t):
    capi.call("pc_tail6_weights", ptr(wf), N, Ci, ptr(W6f), ptr(W6t), stream())


def tail6_gather(cols, bc, bsm, N, It, Ih, Iw, out):
    capi.call("pc_tail6_gather", ptr(cols), ptr(bc), ptr(bsm), N, It, Ih, Iw, ptr(out), stream())
    return out


def tail6_scatter(dout, N, It, Ih, Iw, dcols):
    capi.call("pc_tail6_scatter", ptr(dout), N, It, Ih, Iw, ptr(dcols), stream())
    return dcols


def tail6_wgrad_map(dW6, N, Ci, Gc):
    capi.call("pc_tail6_wgrad_map", ptr(dW6), N, Ci, ptr(Gc), stream())
    return Gc


def tail6_bias_sums(dout, N, It, Ih, Iw, sums, ws=None):
    """ws (tail6_bias_sums_ws_floats floats): per-block partial rows added in block order instead of fp32 atomics."""
    if ws is None:
        capi.call("pc_tail6_bias_sums", ptr(dout), N, It, Ih, Iw, ptr(sums), stream())
    else:
        assert ws.numel() >= tail6_bias_sums_ws_floats(N, It, Ih, Iw)
        capi.call("pc_tail6_bias_sums_ws", ptr(dout), N, It, Ih, Iw, ptr(sums), ptr(ws), stream())
    return sums


def tail6_bias_sums_ws_floats(N, It, Ih, Iw):
    return int(capi.lib().pc_tail6_bias_sums_ws_floats(N, It, Ih, Iw))


def tail6_wgrad_map_slices(ws, nslices8, N, Ci, Gc):
    """ws: the classes' K-slice workspaces back to back ([z][k < nslices8[z]][N][Ci][128], pc_wgrad_desc.ws_slices); a class's image 0 holds the
    class's in-order sum afterwards."""
    import ctypes
    import numpy as np
    ns = np.ascontiguousarray(nslices8, dtype=np.int32)
    assert ns.shape == (8,) and ws.numel() >= int(ns.sum()) * N * Ci * 128
    capi.call("pc_tail6_wgrad_map_slices", ptr(ws), ns.ctypes.data_as(ctypes.c_void_p), N, Ci, ptr(Gc), stream())
    return Gc


def transpose_multi(jobs):
    """jobs: list of (src, dst, batch, R, C, src_batch_stride, src_ld, dst_batch_stride, dst_ld, accum) with torch tensors
    for src / dst: dst[b][c][r] (+)= src[b][r][c] for all of them in one launch."""
    import numpy as np
    tab = np.zeros(len(jobs), dtype=capi.TJOB_DTYPE)
    for q, job in enumerate(jobs):
        src, dst, batch, R, Cc, sbs, sld, dbs, dld, accum = job[:10]
        nslices, sst = (job[10], job[11]) if len(job) > 10 else (0, 0)       # K-slice images of a weight gradient, added in slice order on the way
        if not (src.is_cuda and dst.is_cuda):
            raise RuntimeError("picons ops need CUDA/HIP tensors (no CPU fallback)")
        tab[q] = (src.data_ptr(), dst.data_ptr(), sbs, dbs, batch, R, Cc, sld, dld, int(accum), int(nslices), 0, int(sst))
    capi.call("pc_transpose_multi", C.c_void_p(tab.ctypes.data), len(jobs), stream())


def _lane_array(side):
    """(c_void_p array, n): torch's current stream as lane 0 + the caller's side streams."""
    hs = [torch.cuda.current_stream().cuda_stream] + [st.cuda_stream for st in (side or ())]
    return (C.c_void_p * len(hs))(*hs), len(hs)


def streams_fanin(target, side=None):
    """`target` (a torch stream) waits for everything enqueued so far on torch's current stream and on the side streams."""
    arr, nl = _lane_array(side)
    capi.call("pc_streams_fanin", C.c_void_p(target.cuda_stream), arr, nl)


def run_ops(ops_np, n=None, side=None):
    """ops_np: numpy array of capi.OP_DTYPE (host memory); replayed by the library.  side: extra
    torch.cuda.Stream objects for the plan's lanes 1.. (None -> everything on the current stream)."""
    n = len(ops_np) if n is None else n
    if not side:
        capi.call("pc_run_ops", C.c_void_p(ops_np.ctypes.data), n, stream())
    else:
        arr, nl = _lane_array(side)
        capi.call("pc_run_ops_lanes", C.c_void_p(ops_np.ctypes.data), n, arr, nl)


def run_ops_timed(ops_np, kind, side=None, defer=False):
    """defer: record the event pairs but do not synchronise; timed_collect() reads them later."""
    ms = C.c_float(0); cnt = C.c_int32(0)
    arr, nl = _lane_array(side)
    capi.call("pc_run_ops_timed", C.c_void_p(ops_np.ctypes.data), len(ops_np), kind, None if defer else C.byref(ms), C.byref(cnt), arr, nl)
    return ms.value, cnt.value


def timed_collect():
    ms = C.c_float(0); cnt = C.c_int32(0)
    capi.call("pc_run_ops_timed_collect", C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def seg_frame_counts(logits, gt):
    """logits / gt: contiguous float32 device tensors with the same number of elements, frame-major ([..., H, W] with any
    leading dims flattened to frames).  -> int32 [nframes, 3] = (intersection, union, truth pixels) per frame."""
    if logits.dtype != torch.float32 or gt.dtype != torch.float32 or not logits.is_contiguous() or not gt.is_contiguous():
        raise ValueError("seg_frame_counts: contiguous float32 tensors")
    pix = logits.shape[-1] * logits.shape[-2]
    nframes = logits.numel() // pix
    if gt.numel() != logits.numel():
        raise ValueError("seg_frame_counts: %d logits vs %d truth pixels" % (logits.numel(), gt.numel()))
    counts = torch.empty(nframes, 3, dtype=torch.int32, device=logits.device)
    capi.call("pc_seg_frame_counts", ptr(logits), ptr(gt), nframes, pix, ptr(counts), stream())
    return counts


def map_accumulate(counts, label, frame_hits, video_hits, n_frames, n_vids):
    capi.call("pc_map_accumulate", ptr(counts), counts.shape[0], int(label), frame_hits.shape[0], ptr(frame_hits), ptr(video_hits),
              ptr(n_frames), ptr(n_vids), stream())


VAL_SCALARS = ("total", "loc", "cls", "abs_cls", "bce", "dice", "iou_sum", "iou_clips")     # words 0..7 of a pc_val_metrics record (float32)
VAL_HEAD = 10                                                                                # then n_correct, B (int32), then [B][3] counts


def val_record_words(B):
    return int(capi.lib().pc_val_record_words(int(B)))


def val_metrics_ws_floats(B, pix):
    return int(capi.lib().pc_val_metrics_ws_floats(int(B), int(pix)))


def val_metrics(output, loc_msk, predicted_action, action, record=None, ws=None):
    """pc_val_metrics: output / loc_msk contiguous float32 device tensors (B, ..., H, W) of equal size, predicted_action (B, C) float32,
    action (B,) int32 -> int32 record of val_record_words(B) words (words 0..7 are float32 bit patterns: decode_val_record)."""
    for t in (output, loc_msk, predicted_action):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("val_metrics: contiguous float32 tensors")
    if action.dtype != torch.int32 or not action.is_contiguous():
        raise ValueError("val_metrics: action must be contiguous int32")
    B, C_ = predicted_action.shape
    if output.shape[0] != B or loc_msk.numel() != output.numel() or action.numel() != B:
        raise ValueError("val_metrics: %s logits, %s truth, %s scores, %s actions" % (tuple(output.shape), tuple(loc_msk.shape), (B, C_), tuple(action.shape)))
    pix = output.numel() // B
    if record is None:
        record = torch.empty(max(val_record_words(B), 1), dtype=torch.int32, device=output.device)
    if ws is None:
        ws = torch.empty(max(val_metrics_ws_floats(B, pix), 4), dtype=torch.float32, device=output.device)
    capi.call("pc_val_metrics", ptr(output), ptr(loc_msk), ptr(predicted_action), ptr(action), B, pix, C_, ptr(record), ptr(ws), stream())
    return record


def decode_val_record(rec):
    """One record (host int32 array, numpy or torch) -> dict: the eight float scalars by name, n_correct, B, counts int32 [B][3]."""
    r = _host_words(rec)
    B = int(r[9])
    out = {k: float(v) for k, v in zip(VAL_SCALARS, r[:8].view(np.float32))}
    out.update(n_correct=int(r[8]), B=B, counts=r[VAL_HEAD:VAL_HEAD + 3 * B].reshape(B, 3).copy())
    return out


def clip_from_u8(video, span, h0, w0, rects, S=224, out=None, ndhwc4=False):
    """video: uint8 device tensor [F,H,W,3]; span: 8 frame ids; rects: int32 device tensor [8,R,4] (x0,x1,y0,y1) or None.
    -> data, aug [3,8,S,S] float32, mask [8,S,S] float32 (pc_clip_from_u8).  out: (data, aug, mask) contiguous float32 device tensors of those
    sizes to write into -- a sample's place in a minibatch staging buffer -- instead of fresh ones.  ndhwc4: data / aug as [8,S,S,4] (r, g, b, 0),
    the layout the network's first conv reads (pc_clip_from_u8_ndhwc4)."""
    if video.dtype != torch.uint8 or video.dim() != 4 or video.shape[3] != 3 or not video.is_contiguous():
        raise ValueError("clip_from_u8: contiguous uint8 [F,H,W,3] frames")
    F, H, W, _ = video.shape
    R = 0 if rects is None else int(rects.shape[1])
    if rects is not None and (rects.dtype != torch.int32 or not rects.is_contiguous() or rects.shape[0] != 8 or rects.shape[2] != 4):
        raise ValueError("clip_from_u8: rects must be contiguous int32 [8,R,4]")
    nch = 4 if ndhwc4 else 3
    if out is None:
        data = torch.empty((8, S, S, 4) if ndhwc4 else (3, 8, S, S), device=video.device); aug = torch.empty_like(data); mask = torch.empty(8, S, S, device=video.device)
    else:
        data, aug, mask = out
        for t, n_ in ((data, nch * 8 * S * S), (aug, nch * 8 * S * S), (mask, 8 * S * S)):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n_ or t.device != video.device:
                raise ValueError("clip_from_u8: out tensors must be contiguous float32 device tensors of %d*8*S*S / %d*8*S*S / 8*S*S elements" % (nch, nch))
    sp = (C.c_int32 * 8)(*[int(v) for v in span])
    capi.call("pc_clip_from_u8_ndhwc4" if ndhwc4 else "pc_clip_from_u8", ptr(video), F, H, W, sp, int(h0), int(w0), S, ptr(rects) if R else None, R, ptr(data), ptr(aug), ptr(mask), stream())
    return data, aug, mask


def clip_from_u8_masks(video, span, h0, w0, maskframes, valid, S=224):
    """JHMDB form (pc_clip_from_u8_masks): maskframes uint8 device [F,H,W]; valid: 8 flags.  -> data, aug, mask, mask_cls."""
    if video.dtype != torch.uint8 or video.dim() != 4 or video.shape[3] != 3 or not video.is_contiguous():
        raise ValueError("clip_from_u8_masks: contiguous uint8 [F,H,W,3] frames")
    F, H, W, _ = video.shape
    if maskframes.dtype != torch.uint8 or tuple(maskframes.shape) != (F, H, W) or not maskframes.is_contiguous():
        raise ValueError("clip_from_u8_masks: maskframes must be contiguous uint8 [F,H,W]")
    data = torch.empty(3, 8, S, S, device=video.device); aug = torch.empty_like(data)
    mask = torch.empty(8, S, S, device=video.device); mask_cls = torch.empty_like(mask)
    sp = (C.c_int32 * 8)(*[int(v) for v in span]); va = (C.c_int32 * 8)(*[int(bool(v)) for v in valid])
    capi.call("pc_clip_from_u8_masks", ptr(video), F, H, W, sp, int(h0), int(w0), S, ptr(maskframes), va, ptr(data), ptr(aug), ptr(mask), ptr(mask_cls), stream())
    return data, aug, mask, mask_cls


def _operand(who, name, t, dtypes, n=None, dev=None, dim=None, exact=True, what=""):
    """The operand check of the eval / detect wrappers.  The library refuses nulls, ranges, alignment and the sizes it is told; what it cannot
    see behind a pointer is checked here: `t` is a tensor, of one of `dtypes`, contiguous, of exactly (exact=False: at least) n elements, of
    `dim` dimensions (an int, or a tuple of the allowed ones) and on `dev` -- n, dim and dev where they are given -- or ValueError naming the
    wrapper and the operand (`what`: the layout or the shape, for the message).  -> t."""
    if (isinstance(t, torch.Tensor) and (t.dtype in dtypes if type(dtypes) is tuple else t.dtype == dtypes) and t.is_contiguous()
            and (n is None or (t.numel() == n if exact else t.numel() >= n)) and (dim is None or (t.dim() in dim if type(dim) is tuple else t.dim() == dim))
            and (dev is None or t.device == dev)):
        return t                                                       # (every launch passes here: nothing is formatted on the way)
    raise ValueError("%s: %s must be a contiguous %s tensor%s%s%s%s" % (
        who, name, str(dtypes).replace("torch.", ""), "" if dim is None else " of %s dimensions" % (dim,),
        "" if n is None else " of %s %d elements" % ("exactly" if exact else "at least", n), "" if dev is None else " on %s" % dev,
        what and " (%s)" % (what if isinstance(what, str) else list(what))))


def _frames(who, name, t, dtypes=torch.uint8):
    """A map the wrapper reads its sizes from: _operand with three dimensions -> F, H, W."""
    return (int(v) for v in _operand(who, name, t, dtypes, dim=3, what="[F,H,W]").shape)


def _buffer(who, name, t, shape, dtypes, dev, fill=True, exact=True, n=None):
    """A tensor the launch writes: a given one checked (_operand: n elements, by default those of `shape`, on dev), a missing one made on dev
    with `shape` and the first of `dtypes`, zero-filled -- fill=False: as the allocator leaves it, for a launch that writes all of it."""
    if t is None:
        return (torch.zeros if fill else torch.empty)(shape, dtype=dtypes[0] if isinstance(dtypes, tuple) else dtypes, device=dev)
    if n is None:
        n = 1
        for s in shape:
            n *= int(s)
    return _operand(who, name, t, dtypes, n, dev, exact=exact, what=shape)


def _workspace(who, ws, need, dev, ws_call, any_dtype=False):
    """The scratch of a launch that needs `need` bytes (ws_call: the size function, for the message): a given one checked -- contiguous uint8 of
    at least `need` elements on dev; any_dtype=True (the detect_frames family): any dtype, by its bytes -- a missing one made, None for no
    bytes."""
    if ws is None:
        return torch.empty(need, dtype=torch.uint8, device=dev) if need > 0 else None
    if any_dtype and torch.is_tensor(ws):
        return _operand(who, "ws", ws, ws.dtype, -(-need // ws.element_size()), dev, exact=False, what=ws_call)
    return _operand(who, "ws", ws, torch.uint8, need, dev, exact=False, what=ws_call)


def _ws_bytes(name, limits, *args, tail=()):
    """pc_<name>(*args), host arithmetic in the library -> the bytes of workspace; ValueError (`limits` % (args + tail): what the sizes must
    keep to) where it answers -1."""
    n = int(getattr(capi.lib(), "pc_" + name)(*map(int, args)))
    if n < 0:
        raise ValueError("%s: %s" % (name, limits % (args + tail)))
    return n


def _frame_range(who, F, f0, nf, refuse=True):
    """The frames f0 .. f0 + nf - 1 of F (nf=None: all from f0 on) -> f0, nf as ints.  refuse=False leaves a range outside the F frames to the
    library (RuntimeError); else it is a ValueError here, in front of the buffers the range sizes."""
    f0 = int(f0)
    nf = F - f0 if nf is None else int(nf)
    if refuse and (f0 < 0 or nf < 1 or f0 + nf > F):
        raise ValueError("%s: frames f0 = %d, nf = %d outside the %d of the map" % (who, f0, nf, F))
    return f0, nf


def _bound(who, name, v, hi):
    """A count the buffers are sized by -> int(v) in 1..hi, or ValueError."""
    v = int(v)
    if not 1 <= v <= hi:
        raise ValueError("%s: %s = %d outside 1..%d" % (who, name, v, hi))
    return v


def _host_words(x, dtype=np.int32):
    """What the decode_* functions take (a host array, numpy or torch) -> contiguous numpy of `dtype` (None: its own)."""
    return np.ascontiguousarray(x.cpu().numpy() if torch.is_tensor(x) else x, dtype=dtype)


_HOST_TABLES = {}


def _host_table(entry, args, device=None, refuse=None):
    """A table the library computes on the host, by its size-then-fill protocol: entry(*args, NULL, 0) -> the int32 words it takes, then
    entry(*args, buffer, words) fills them.  device=None: -> the numpy array.  Else -> the table on that device, cached per (entry, args,
    device).  Arguments the entry does not take: ValueError(refuse), without one the library's own RuntimeError."""
    key = (entry, args, device if device is None else str(torch.device(device)))
    tab = _HOST_TABLES.get(key)
    if tab is None:
        fn = getattr(capi.lib(), entry)
        need = int(fn(*args, None, 0))
        if need < 0 and refuse:
            raise ValueError(refuse)
        if need < 0:
            capi.check(need)
        tab = np.zeros(need, np.int32)
        got = fn(*args, C.c_void_p(tab.ctypes.data), need)
        assert got == need
        if device is not None:
            tab = _HOST_TABLES[key] = torch.from_numpy(tab).to(device)
    return tab


def _u8_video(video, who, truth=None):
    """The video check of the clip-cut wrappers (and the truth's, where one comes with it) -> F, H, W."""
    if _operand(who, "video", video, torch.uint8, dim=4, what="[F,H,W,3] frames").shape[3] != 3:
        raise ValueError("%s: contiguous uint8 [F,H,W,3] frames" % who)
    if truth is not None:
        _operand(who, "truth", truth, torch.uint8, video.numel() // 3, what="[F,H,W] of the video's size")
        if tuple(truth.shape[:3]) != tuple(video.shape[:3]):
            raise ValueError("%s: truth must be contiguous uint8 [F,H,W] of the video's size" % who)
    return (int(v) for v in video.shape[:3])


def _starts_table(starts):
    """First-frame indices (host) -> (the int32 table the clip entries take, n)."""
    n = len(starts)
    return (C.c_int32 * max(n, 1))(*[int(v) for v in starts]), n


def truth_frame_flags(truth, h0, w0, S, flags=None):
    """pc_truth_frame_flags: truth uint8 device [F,H,W] -> int32 [F], the non-zero truth pixels of each frame inside the S x S crop at (h0, w0).
    flags: an int32 device tensor of at least F elements to write into."""
    F, H, W = _frames("truth_frame_flags", "truth", truth)
    if flags is None:
        flags = torch.empty(F, dtype=torch.int32, device=truth.device)
    else:
        _operand("truth_frame_flags", "flags", flags, torch.int32, F, exact=False)
    capi.call("pc_truth_frame_flags", ptr(truth), F, H, W, int(h0), int(w0), int(S), ptr(flags), stream())
    return flags[:F]


def eval_clips_from_u8(video, truth, h0, w0, S, starts, f_skip=2, out=None):
    """pc_eval_clips_from_u8: video uint8 device [F,H,W,3], truth uint8 device [F,H,W]; starts: 1..32 first-frame indices (host).
    -> data [n,8,S,S,4] float32 (r, g, b, 0), gt [n,8,S,S] float32 (the truth values; zero frames past the end).  out: (data, gt) contiguous
    float32 device tensors with room for n clips -- a batch's place in the plan's clip tensor -- instead of fresh ones."""
    F, H, W = _u8_video(video, "eval_clips_from_u8", truth)
    st, n = _starts_table(starts)
    data, gt = (None, None) if out is None else out
    data = _buffer("eval_clips_from_u8", "out[0]", data, (n, 8, S, S, 4), torch.float32, video.device, fill=False, exact=False)
    gt = _buffer("eval_clips_from_u8", "out[1]", gt, (n, 8, S, S), torch.float32, video.device, fill=False, exact=False)
    capi.call("pc_eval_clips_from_u8", ptr(video), ptr(truth), F, H, W, int(h0), int(w0), int(S), st, n, int(f_skip), ptr(data), ptr(gt), stream())
    return data, gt


def video_vote(pred, label, n_correct):
    """pc_video_vote: n_correct (int32 device, 1 element) += argmax(mean(pred, axis=0)) == label; pred contiguous float32 device [n,C]."""
    _operand("video_vote", "pred", pred, torch.float32, dim=2, what="[n,C] scores")
    if n_correct.dtype != torch.int32 or n_correct.numel() < 1:      # only its first element is touched: any stride will do
        raise ValueError("video_vote: n_correct must be an int32 device tensor")
    capi.call("pc_video_vote", ptr(pred), int(pred.shape[0]), int(pred.shape[1]), int(label), ptr(n_correct), stream())


def clips_from_u8(video, h0, w0, S, starts, f_skip=2, out=None):
    """pc_clips_from_u8: eval_clips_from_u8 without truth.  video uint8 device [F,H,W,3]; starts: 1..32 first-frame indices (host).
    -> data [n,8,S,S,4] float32 (r, g, b, 0).  out: a contiguous float32 device tensor with room for n clips to write into."""
    F, H, W = _u8_video(video, "clips_from_u8")
    st, n = _starts_table(starts)
    out = _buffer("clips_from_u8", "out", out, (n, 8, S, S, 4), torch.float32, video.device, fill=False, exact=False)
    capi.call("pc_clips_from_u8", ptr(video), F, H, W, int(h0), int(w0), int(S), st, n, int(f_skip), ptr(out), stream())
    return out


DETECT_REC_WORDS = 8        # a pc_detect_frames record: count, x0, y0, x1, y1, float32 score bits, clip row, 0


def detect_frames_ws_bytes(n, S):
    return int(capi.lib().pc_detect_frames_ws_bytes(int(n), int(S)))


def _detect_buffers(who, dev, F, H, W, mask, rec, ws, want_mask, ws_call, need, any_ws=True):
    """The mask / rec / ws of the detect_frames family and prob_cut: given ones checked, missing ones made (mask and rec zero-filled; no mask
    with want_mask=False).  ws_call names the size function in the message; need: its value; any_ws: _workspace's any_dtype.
    -> mask, rec, ws."""
    if mask is not None or want_mask:
        mask = _buffer(who, "mask", mask, (F, H, W), torch.uint8, dev)
    rec = _buffer(who, "rec", rec, (F, DETECT_REC_WORDS), torch.int32, dev)
    return mask, rec, _workspace(who, ws, need, dev, ws_call, any_ws)


def detect_frames(logits, starts, F, H, W, h0, w0, f_skip=2, row0=0, mask=None, rec=None, ws=None, want_mask=True):
    """pc_detect_frames: logits contiguous float32 device [n,8,S,S] (any shape with those elements; S from the last dim), the eval forward's
    output for the n <= 32 clips of one video cut at `starts`.  -> (mask uint8 [F,H,W] or None, rec int32 [F,8]); given tensors are written
    in place -- only the frames the clips address -- fresh ones are zero-filled first.  want_mask=False with mask=None: records only."""
    _tab, _V, st, n, S, _stride = _clip_logits("detect_frames", logits, None, starts, None)
    mask, rec, ws = _detect_buffers("detect_frames", logits.device, F, H, W, mask, rec, ws, want_mask, "detect_frames_ws_bytes(n, S)",
                                    detect_frames_ws_bytes(n, S))
    capi.call("pc_detect_frames", ptr(logits), int(F), int(H), int(W), int(h0), int(w0), S, st, n, int(f_skip), int(row0), ptr(mask), ptr(rec),
              ptr(ws), stream())
    return mask, rec


MAX_VIEWS = 32              # views of one pc_clips_from_u8_views / pc_detect_frames_views launch (csrc/clipgeom.h); detect.py takes it from here


def _view_table(views, who):
    """[(h0, w0, flip)] -> (the host table int32 [V][3] the views entries take, V)."""
    rows = [tuple(int(x) for x in v) for v in views]
    if not 1 <= len(rows) <= MAX_VIEWS or any(len(r) != 3 for r in rows):
        raise ValueError("%s: 1..%d views (h0, w0, flip), got %r" % (who, MAX_VIEWS, views))
    return (C.c_int32 * (3 * len(rows)))(*[x for r in rows for x in r]), len(rows)


def _view_stride(who, view_stride, n):
    """The clip slots between two views of one clip (default: the n clips) -> int, or ValueError below n."""
    stride = n if view_stride is None else int(view_stride)
    if stride < n:
        raise ValueError("%s: view_stride = %d below the %d clips" % (who, stride, n))
    return stride


def _clip_logits(who, logits, views, starts, view_stride):
    """The opening of the entries that take a forward's logits: contiguous float32 (S from the last dim) that hold view v of clip c at clip slot
    v * view_stride + c (default stride: n = len(starts)).  views=None: the centre entry, which has no view table and one view.
    -> (view table or None, V, starts table, n, S, view_stride)."""
    _operand(who, "logits", logits, torch.float32)
    tab, V = (None, 1) if views is None else _view_table(views, who)
    st, n = _starts_table(starts)
    S = int(logits.shape[-1])
    stride = _view_stride(who, view_stride, n)
    if int(logits.shape[-2]) != S or logits.numel() < ((V - 1) * stride + n) * 8 * S * S:
        if views is None:
            raise ValueError("%s: logits %s do not hold %d clips of 8 x %d x %d" % (who, tuple(logits.shape), n, S, S))
        raise ValueError("%s: logits %s do not hold %d views of %d clips of 8 x %d x %d at stride %d" % (who, tuple(logits.shape), V, n, S, S, stride))
    return tab, V, st, n, S, stride


def clips_from_u8_views(video, views, S, starts, f_skip=2, view_stride=None, out=None):
    """pc_clips_from_u8_views: clips_from_u8 for every view (h0, w0, flip) of the n <= 32 clips in one launch.  View v of clip c is written at
    clip slot v * view_stride + c (view_stride >= n, default n).  -> data [V, view_stride, 8, S, S, 4] float32, or `out` (a contiguous float32
    device tensor with room for (V - 1) * view_stride + n clips) as it was given; the slots between the views are not written."""
    F, H, W = _u8_video(video, "clips_from_u8_views")
    tab, V = _view_table(views, "clips_from_u8_views")
    st, n = _starts_table(starts)
    stride = _view_stride("clips_from_u8_views", view_stride, n)
    out = _buffer("clips_from_u8_views", "out", out, (V, stride, 8, S, S, 4), torch.float32, video.device, fill=False, exact=False,
                  n=((V - 1) * stride + n) * 32 * S * S)
    capi.call("pc_clips_from_u8_views", ptr(video), F, H, W, int(S), tab, V, stride, st, n, int(f_skip), ptr(out), stream())
    return out


def detect_frames_views_ws_bytes(n, H, W):
    return int(capi.lib().pc_detect_frames_views_ws_bytes(int(n), int(H), int(W)))


def detect_frames_views(logits, views, starts, F, H, W, f_skip=2, view_stride=None, row0=0, mask=None, rec=None, ws=None, want_mask=True):
    """pc_detect_frames_views: detect_frames with the views (h0, w0, flip) of every clip merged per full-frame pixel.  logits contiguous float32
    device (S from the last dim), view v of clip c at clip slot v * view_stride + c (default stride: n = len(starts)).
    -> (mask uint8 [F,H,W] or None, rec int32 [F,8]) as detect_frames; rec[:, 6] = row0 + c * V."""
    tab, V, st, n, S, stride = _clip_logits("detect_frames_views", logits, views, starts, view_stride)
    mask, rec, ws = _detect_buffers("detect_frames_views", logits.device, F, H, W, mask, rec, ws, want_mask, "detect_frames_views_ws_bytes(n, H, W)",
                                    detect_frames_views_ws_bytes(n, H, W))
    capi.call("pc_detect_frames_views", ptr(logits), int(F), int(H), int(W), S, tab, V, stride, st, n, int(f_skip), int(row0), ptr(mask), ptr(rec),
              ptr(ws), stream())
    return mask, rec


def resample_tables(Hs, Ws, H, W, device):
    """pc_resample_tables(Hs, Ws, H, W) on the device: int32 [2 * (H + W)], rows [H][2] then columns [W][2] of (first tap, float32 bits of the
    second tap's weight) that take a working frame of Hs x Ws back to the native H x W.  Host arithmetic in the library, cached per sizes and
    device."""
    return _host_table("pc_resample_tables", (int(Hs), int(Ws), int(H), int(W)), device)


def _native_buffers(who, dev, F, H, W, Hs, Ws, mask, prob, rec, ws, want_mask, ws_call, need):
    """What the entries that detect at native size from an Hs x Ws plane write and read besides it: _detect_buffers, a given prob checked,
    the tables on the device.  -> mask, prob, rec, ws, dev_tab."""
    mask, rec, ws = _detect_buffers(who, dev, F, H, W, mask, rec, ws, want_mask, ws_call, need)
    if prob is not None:
        _buffer(who, "prob", prob, (F, H, W), _PROB_DTYPES, dev)
    return mask, prob, rec, ws, resample_tables(Hs, Ws, H, W, dev)


def detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W):
    return int(capi.lib().pc_detect_frames_scaled_ws_bytes(int(n), int(Hs), int(Ws), int(H), int(W)))


def detect_frames_scaled(logits, views, starts, F, H, W, Hs, Ws, f_skip=2, view_stride=None, row0=0, mask=None, prob=None, rec=None, ws=None,
                         want_mask=True):
    """pc_detect_frames_scaled: detect_frames_views for views (h0, w0, flip) that are crops of an Hs x Ws WORKING frame, the merged logits
    resampled bilinearly to every pixel of the native H x W frame in front of the threshold, the box, the score and the probability.
    -> (mask uint8 [F,H,W] or None, rec int32 [F,8]) as detect_frames_views, in native coordinates; prob: a 16-bit integer device tensor
    [F,H,W] the same launch fills as frame_probs would (only the frames the clips address), or None for none."""
    tab, V, st, n, S, stride = _clip_logits("detect_frames_scaled", logits, views, starts, view_stride)
    F, H, W, Hs, Ws = int(F), int(H), int(W), int(Hs), int(Ws)
    need = detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W)
    if need < 0:
        raise ValueError("detect_frames_scaled: %d clips, working frame %d x %d, native frame %d x %d" % (n, Hs, Ws, H, W))
    mask, prob, rec, ws, dev_tab = _native_buffers("detect_frames_scaled", logits.device, F, H, W, Hs, Ws, mask, prob, rec, ws, want_mask,
                                                   "detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W)", need)
    capi.call("pc_detect_frames_scaled", ptr(logits), F, H, W, Hs, Ws, S, tab, V, stride, st, n, int(f_skip), int(row0), ptr(dev_tab), ptr(mask),
              ptr(prob), ptr(rec), ptr(ws), stream())
    return mask, rec


PLANES_MAX_FRAMES = 256     # PC_PLANES_MAX_FRAMES of include/picons.h: the frames of one pc_detect_frames_planes range


def clip_hop_starts(F, f_skip, hop):
    """pc_clip_hop_starts: the clip starts of a video of F frames cut into windows of 8 * f_skip frames every `hop` frames (host arithmetic
    in the library; csrc/cliphop.h states the rule) -> list of ints.  ValueError for F < 1 or a hop that is no multiple of f_skip in
    [f_skip, 8 * f_skip]."""
    args = (int(F), int(f_skip), int(hop))
    return _host_table("pc_clip_hop_starts", args, refuse="clip_hop_starts: F = %d, f_skip = %d, hop = %d" % args).tolist()


def clip_planes_bytes(F, Hs, Ws, f_skip, hop):
    """pc_clip_planes_bytes: the bytes of a video's slot planes float32 [M][F][pstride] and, behind them, its cover bytes [pstride]; -1 for
    sizes or a hop the library does not take."""
    return int(capi.lib().pc_clip_planes_bytes(int(F), int(Hs), int(Ws), int(f_skip), int(hop)))


def clip_plane_views(planes, F, Hs, Ws, f_skip, hop):
    """The two parts of a clip_planes buffer -> (plane float32 [M, F, pstride], cover uint8 [pstride]), views of `planes`."""
    need = clip_planes_bytes(F, Hs, Ws, f_skip, hop)
    if need < 0:
        raise ValueError("clip_planes: %d frames of %d x %d, f_skip = %d, hop = %d" % (F, Hs, Ws, f_skip, hop))
    _operand("clip_planes", "planes", planes, torch.uint8, need, exact=False, what="clip_planes_bytes(F, Hs, Ws, f_skip, hop) = %d bytes" % need)
    ps = clip_planes_bytes(1, Hs, Ws, 1, 8) // 5                    # the library's own stride: one frame in one slot is 4 * ps + ps bytes
    M = (need - ps) // (4 * int(F) * ps)
    return planes[:need - ps].view(torch.float32).view(M, int(F), ps), planes[need - ps:need]


def clip_planes(logits, views, starts, F, Hs, Ws, f_skip, hop, view_stride=None, planes=None, cover=True):
    """pc_clip_planes: the logits, views and starts of detect_frames_views for n <= 32 clips of one video cut at `hop` -> `planes`, a uint8
    device tensor of clip_planes_bytes(F, Hs, Ws, f_skip, hop): frame k of clip c as the merged logits of the Hs x Ws frame in slot
    (starts[c] / hop) % M of frame starts[c] + k * f_skip.  cover=True: the launch also writes the cover bytes (a video's first launch).  A
    given buffer is written in place -- only the (slot, frame) pairs the clips address; a fresh one is NOT filled."""
    tab, V, st, n, S, stride = _clip_logits("clip_planes", logits, views, starts, view_stride)
    F, Hs, Ws, f_skip, hop = int(F), int(Hs), int(Ws), int(f_skip), int(hop)
    need = clip_planes_bytes(F, Hs, Ws, f_skip, hop)
    if need < 0:
        raise ValueError("clip_planes: %d frames of %d x %d, f_skip = %d, hop = %d" % (F, Hs, Ws, f_skip, hop))
    if planes is None:
        planes = torch.empty(need, dtype=torch.uint8, device=logits.device)
    elif planes.device != logits.device:
        raise ValueError("clip_planes: planes must be on the logits' device")
    plane, cov = clip_plane_views(planes, F, Hs, Ws, f_skip, hop)
    capi.call("pc_clip_planes", ptr(logits), F, Hs, Ws, S, tab, V, stride, st, n, f_skip, hop, ptr(plane), ptr(cov) if cover else None, stream())
    return planes


def detect_frames_planes_ws_bytes(nf, H, W):
    return int(capi.lib().pc_detect_frames_planes_ws_bytes(int(nf), int(H), int(W)))


def detect_frames_planes(planes, F, H, W, Hs, Ws, V, f_skip, hop, f0=0, nf=None, row0=0, mask=None, prob=None, rec=None, ws=None, want_mask=True):
    """pc_detect_frames_planes: the buffer clip_planes filled for every clip of a video -> the frames f0 .. f0 + nf - 1 (nf at most
    PLANES_MAX_FRAMES; default: the rest of the video) detected at native size from the mean of the windows that hold each frame.
    -> (mask uint8 [F,H,W] or None, rec int32 [F,8]) as detect_frames_scaled, rec[:, 6] = row0 + V * (the first clip that holds the frame);
    prob as there.  Given tensors are written in place -- only the frames of the range -- fresh ones are zero-filled first."""
    F, H, W, Hs, Ws = int(F), int(H), int(W), int(Hs), int(Ws)
    f0, nf = _frame_range("detect_frames_planes", F, f0, nf, refuse=False)
    plane, cov = clip_plane_views(planes, F, Hs, Ws, f_skip, hop)
    need = detect_frames_planes_ws_bytes(nf, H, W)
    if need < 0 or f0 < 0 or f0 + nf > F:
        raise ValueError("detect_frames_planes: frames %d .. %d + %d of %d (a range holds 1..%d), native frame %d x %d" % (f0, f0, nf, F, PLANES_MAX_FRAMES, H, W))
    mask, prob, rec, ws, dev_tab = _native_buffers("detect_frames_planes", planes.device, F, H, W, Hs, Ws, mask, prob, rec, ws, want_mask,
                                                   "detect_frames_planes_ws_bytes(nf, H, W)", need)
    capi.call("pc_detect_frames_planes", ptr(plane), ptr(cov), F, H, W, Hs, Ws, int(V), int(f_skip), int(hop), f0, nf, int(row0), ptr(dev_tab), ptr(mask),
              ptr(prob), ptr(rec), ptr(ws), stream())
    return mask, rec


def decode_detect_records(rec):
    """Host int32 [F,8] records (numpy or torch) -> (counts int32 [F], boxes int32 [F,4] = x0, y0, x1, y1, frame_scores float32 [F], rows int32 [F])."""
    r = _host_words(rec).reshape(-1, DETECT_REC_WORDS)
    return r[:, 0].copy(), r[:, 1:5].copy(), r[:, 5].copy().view(np.float32), r[:, 6].copy()


INST_HDR, INST_WORDS = 4, 6                # a pc_frame_instances record: n_comp, kept, n_runs, flags, then K slots of area, x0, y0, x1, y1, first
INST_MAX_RUNS, INST_MAX_ROWS = 2048, 2048  # PC_INST_MAX_RUNS / PC_INST_MAX_ROWS of include/picons.h
INST_MAX_K = 32


def frame_instances(mask, f0=0, nf=None, conn=8, min_area=1, K=8, inst=None, imap=None, want_imap=True):
    """pc_frame_instances: mask contiguous uint8 device [F,H,W] (any non-zero byte is foreground) -> (inst int32 [F, 4 + 6K], imap uint8 [F,H,W]
    or None): the connected components (conn 4 or 8) of the frames f0 .. f0 + nf - 1 (default: all from f0 on), ranked by area.  Given tensors
    are written in place -- only those frames -- fresh ones are zero-filled first.  want_imap=False with imap=None: records only."""
    F, H, W = _frames("frame_instances", "mask", mask)
    K = _bound("frame_instances", "K", K, INST_MAX_K)
    f0, nf = _frame_range("frame_instances", F, f0, nf, refuse=False)
    inst = _buffer("frame_instances", "inst", inst, (F, INST_HDR + K * INST_WORDS), torch.int32, mask.device)
    if imap is not None or want_imap:
        imap = _buffer("frame_instances", "imap", imap, (F, H, W), torch.uint8, mask.device)
    capi.call("pc_frame_instances", ptr(mask), F, H, W, f0, nf, int(conn), int(min_area), K, ptr(inst), ptr(imap), stream())
    return inst, imap


def decode_instances(words, K):
    """Host int32 [F, 4 + 6K] records (numpy or torch) -> (n_comp int32 [F], kept int32 [F], n_runs int32 [F], flags int32 [F], areas int32 [F,K],
    boxes int32 [F,K,4] = x0, y0, x1, y1, first int32 [F,K])."""
    K = int(K)
    r = _host_words(words).reshape(-1, INST_HDR + K * INST_WORDS)
    slots = r[:, INST_HDR:].reshape(-1, K, INST_WORDS)
    return r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy(), slots[:, :, 0].copy(), slots[:, :, 1:5].copy(), slots[:, :, 5].copy()


PROB_ONE, SCORE_WORDS = 65535, 3           # PC_PROB_ONE / PC_SCORE_WORDS of include/picons.h: probability 1.0 as uint16; lo, hi, npix of a slot
# The probability map of frame_probs / instance_scores: a contiguous 16-bit integer device tensor [F,H,W], np.uint16 on the host
# (prob.cpu().numpy().view(np.uint16)).  A missing one is made zero-filled as the first of these, int16: the dtype every torch build can
# allocate and copy.
_PROB_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)


def frame_probs(logits, views, starts, F, H, W, f_skip=2, view_stride=None, prob=None):
    """pc_frame_probs: the logits, views and starts of detect_frames_views (the centre crop: the one view (h0, w0, 0)) -> prob, 16-bit integer
    device [F,H,W]: round(65535 * sigmoid(merged logit)) as uint16, 0 where no view covers the pixel.  A given tensor is written in place
    -- only the frames the clips address -- a fresh one is zero-filled first."""
    tab, V, st, n, S, stride = _clip_logits("frame_probs", logits, views, starts, view_stride)
    prob = _buffer("frame_probs", "prob", prob, (int(F), int(H), int(W)), _PROB_DTYPES, logits.device)
    capi.call("pc_frame_probs", ptr(logits), int(F), int(H), int(W), S, tab, V, stride, st, n, int(f_skip), ptr(prob), stream())
    return prob


def instance_scores(imap, prob, K, f0=0, nf=None, out=None):
    """pc_instance_scores: imap contiguous uint8 device [F,H,W] (frame_instances' map of ranks) and prob (frame_probs') -> out int32
    [F, 3 * (K + 1)]: per slot the 64-bit sum of prob over its pixels as (lo, hi) and their number, for the frames f0 .. f0 + nf - 1
    (default: all from f0 on).  A given out is written in place -- only those frames -- a fresh one is zero-filled first."""
    F, H, W = _frames("instance_scores", "imap", imap)
    K = _bound("instance_scores", "K", K, INST_MAX_K)
    if prob is None:
        raise ValueError("instance_scores: prob is missing")
    _buffer("instance_scores", "prob", prob, (F, H, W), _PROB_DTYPES, imap.device)
    f0, nf = _frame_range("instance_scores", F, f0, nf, refuse=False)
    out = _buffer("instance_scores", "out", out, (F, SCORE_WORDS * (K + 1)), torch.int32, imap.device)
    capi.call("pc_instance_scores", ptr(imap), ptr(prob), F, H, W, f0, nf, K, ptr(out), stream())
    return out


def decode_instance_scores(words, K):
    """Host int32 [F, 3 * (K + 1)] records (numpy or torch) -> (sums int64 [F, K + 1], npix int32 [F, K + 1]); slot K: all other foreground."""
    K = int(K)
    r = _host_words(words).reshape(-1, K + 1, SCORE_WORDS)
    lo, hi = r[:, :, 0].astype(np.int64) & 0xffffffff, r[:, :, 1].astype(np.int64) & 0xffffffff
    return (hi << 32) | lo, r[:, :, 2].copy()


LINK_MAX_LAGS = 4                          # PC_LINK_MAX_LAGS of include/picons.h: the frame distances one overlap record covers


def instance_overlaps(imap, K, L=1, f0=0, nf=None, out=None):
    """pc_instance_overlaps: imap contiguous uint8 device [F,H,W] (frame_instances' map of ranks) -> out int32 [F, L, K + 1, K + 1]:
    out[f, l, a, b] the pixels whose slot is a in frame f and b in frame f + l + 1 (slot K: all other foreground; zeros where that frame
    does not exist), for the frames f0 .. f0 + nf - 1 (default: all from f0 on).  A given out is written in place -- only those frames -- a
    fresh one is zero-filled first."""
    F, H, W = _frames("instance_overlaps", "imap", imap)
    K, L = _bound("instance_overlaps", "K", K, INST_MAX_K), _bound("instance_overlaps", "L", L, LINK_MAX_LAGS)
    f0, nf = _frame_range("instance_overlaps", F, f0, nf, refuse=False)
    out = _buffer("instance_overlaps", "out", out, (F, L, K + 1, K + 1), torch.int32, imap.device)
    capi.call("pc_instance_overlaps", ptr(imap), F, H, W, f0, nf, K, L, ptr(out), stream())
    return out


def decode_instance_overlaps(words, K, L):
    """Host int32 records of F * L * (K + 1)^2 words (numpy or torch, any shape) -> int32 [F, L, K + 1, K + 1]."""
    K, L = int(K), int(L)
    return _host_words(words).reshape(-1, L, K + 1, K + 1).copy()


RUN_WORDS = 2                              # PC_RUN_WORDS of include/picons.h: a run is (row | value << 24, x0 | x1 << 16)
RUN_MAX_ROWS, RUN_MAX_PIXELS = 1 << 24, (1 << 31) - 1      # what one range of pc_mask_run_index / pc_mask_runs may hold


def _run_range(who, map, f0, nf):
    """The map and frame range of mask_run_index / mask_runs -> (F, H, W, f0, nf), or ValueError."""
    F, H, W = _frames(who, "map", map)
    f0, nf = _frame_range(who, F, f0, nf)
    if H < 1 or not 1 <= W <= 65535 or nf * H > RUN_MAX_ROWS or nf * H * W > RUN_MAX_PIXELS:
        raise ValueError("%s: %d frames of %d x %d: W <= 65535, nf * H <= 2^24 and nf * H * W < 2^31 (export a longer video in ranges)" % (who, nf, H, W))
    return F, H, W, f0, nf


def mask_run_index(map, f0=0, nf=None, index=None):
    """pc_mask_run_index: map contiguous uint8 device [F,H,W] -> index int32 device [nf * H + 1] for the frames f0 .. f0 + nf - 1 (default: all
    from f0 on): index[r] the row runs (maximal horizontal segments of one non-zero byte value) in the rows before row r = (f - f0) * H + y,
    index[nf * H] their total.  A given index is written in place, all of it."""
    F, H, W, f0, nf = _run_range("mask_run_index", map, f0, nf)
    index = _buffer("mask_run_index", "index", index, (nf * H + 1,), torch.int32, map.device, fill=False)
    ws = torch.empty(capi.lib().pc_mask_run_ws_bytes(nf, H) // 4, dtype=torch.int32, device=map.device)
    capi.call("pc_mask_run_index", ptr(map), F, H, W, f0, nf, ptr(index), ptr(ws), stream())
    return index


def mask_runs(map, index, f0=0, nf=None, cap=None, runs=None):
    """pc_mask_runs: map and the index mask_run_index made for the same range -> runs int32 device [cap, 2] (uint32 words: int32 is the dtype
    every torch build can allocate and copy; .cpu().numpy().view(np.uint32) on the host) in raster order: (row | value << 24, x0 | x1 << 16).
    cap=None: the range's total is read from the index -- ONE host wait -- and the tensor holds exactly the runs.  A given cap: no wait; runs
    from cap on are not written (compare index[-1] with cap).  A given runs tensor [cap, 2] is written in place."""
    F, H, W, f0, nf = _run_range("mask_runs", map, f0, nf)
    _operand("mask_runs", "index", index, torch.int32, nf * H + 1, map.device, what="[nf * H + 1]")
    if cap is None:
        cap = int(index[-1].item()) if runs is None else runs.numel() // RUN_WORDS
    cap = int(cap)
    if cap < 0:
        raise ValueError("mask_runs: cap = %d below 0" % cap)
    runs = _buffer("mask_runs", "runs", runs, (cap, RUN_WORDS), torch.int32, map.device, fill=False)
    capi.call("pc_mask_runs", ptr(map), F, H, W, f0, nf, ptr(index), cap, ptr(runs), stream())
    return runs


def decode_mask_runs(runs, nf, H, W):
    """Host runs [n, 2] (numpy or torch, int32 or uint32 words) with rows numbered from 0 over nf frames of H rows -> numpy uint8 [nf, H, W]:
    every run's value on its pixels, 0 elsewhere.  ValueError for a run outside the frames."""
    nf, H, W = int(nf), int(H), int(W)
    r = _host_words(runs, None)
    if r.dtype not in (np.int32, np.uint32) or r.size % RUN_WORDS:
        raise ValueError("decode_mask_runs: runs must be 32-bit words [n, %d], got %s %s" % (RUN_WORDS, r.dtype, r.shape))
    r = r.view(np.uint32).reshape(-1, RUN_WORDS)
    row, val = (r[:, 0] & 0xffffff).astype(np.int64), (r[:, 0] >> 24).astype(np.int16)
    x0, x1 = (r[:, 1] & 0xffff).astype(np.int64), (r[:, 1] >> 16).astype(np.int64)
    if r.shape[0] and (row.max() >= nf * H or x1.max() > W or (x0 >= x1).any() or (val == 0).any()):
        raise ValueError("decode_mask_runs: a run outside %d frames of %d x %d, empty, or of value 0" % (nf, H, W))
    # a step up at x0 and down at x1, summed along the row: runs of one row do not overlap, so each (row, x0) and each (row, x1) occurs once
    d = np.zeros((nf * H, W + 1), np.int16)
    d[row, x0] += val
    d[row, x1] -= val
    return np.cumsum(d[:, :W], axis=1, dtype=np.int16).astype(np.uint8).reshape(nf, H, W)


CROSS_MAX_SLOTS = 32                       # PC_CROSS_MAX_SLOTS of include/picons.h: the pred values P and the truth values A with a slot of their own


def map_crosstab_ws_bytes(nf, H, W, P, A):
    """pc_map_crosstab_ws_bytes (host arithmetic): the bytes of workspace one map_crosstab call over nf frames of H x W takes."""
    return _ws_bytes("map_crosstab_ws_bytes", "nf = %d frames of %d x %d with P = %d, A = %d: nf, H, W >= 1, H * W < 2^31, P and A in 1..%d",
                     nf, H, W, P, A, tail=(CROSS_MAX_SLOTS,))


def _same_frames(who, a, ta, b, tb, dtypes=torch.uint8):
    """The two maps [F,H,W] a call holds against each other (ta of `dtypes`, tb uint8): one shape, one device -> F, H, W."""
    _operand(who, a, ta, dtypes, dim=3, what="[F,H,W]")
    _operand(who, b, tb, torch.uint8, dim=3, what="[F,H,W]")
    if ta.shape != tb.shape or ta.device != tb.device:
        raise ValueError("%s: %s %s and %s %s must have one shape and lie on one device" % (who, a, tuple(ta.shape), b, tuple(tb.shape)))
    return (int(v) for v in ta.shape)


def map_crosstab(pred, truth, P, A, f0=0, nf=None, out=None, ws=None):
    """pc_map_crosstab: pred and truth contiguous uint8 device [F,H,W], two different buffers -> out int32 [F, P + 2, A + 2]: out[f, p, a] the
    pixels of frame f with pred slot p (0 background, v for a byte 1..P, P + 1 for any byte above P) and truth slot a (the same with A),
    cell [0, 0] included, for the frames f0 .. f0 + nf - 1 (default: all from f0 on).  A given out is written in place -- only those frames
    -- a fresh one is zero-filled first.  ws: uint8 device scratch of at least map_crosstab_ws_bytes(nf, H, W, P, A) bytes, made when None."""
    F, H, W = _same_frames("map_crosstab", "pred", pred, "truth", truth)
    P, A = _bound("map_crosstab", "P", P, CROSS_MAX_SLOTS), _bound("map_crosstab", "A", A, CROSS_MAX_SLOTS)
    f0, nf = _frame_range("map_crosstab", F, f0, nf)
    out = _buffer("map_crosstab", "out", out, (F, P + 2, A + 2), torch.int32, pred.device)
    ws = _workspace("map_crosstab", ws, map_crosstab_ws_bytes(nf, H, W, P, A), pred.device, "map_crosstab_ws_bytes(nf, H, W, P, A)")
    capi.call("pc_map_crosstab", ptr(pred), ptr(truth), F, H, W, f0, nf, P, A, ptr(out), ptr(ws), stream())
    return out


def decode_map_crosstab(words, P, A):
    """Host int32 tables of F * (P + 2) * (A + 2) words (numpy or torch, any shape) -> int32 [F, P + 2, A + 2]."""
    P, A = int(P), int(A)
    return _host_words(words).reshape(-1, P + 2, A + 2).copy()


SWEEP_MAX_THRESHOLDS = 64                  # PC_SWEEP_MAX_THRESHOLDS of include/picons.h: the threshold words one histogram is split by


def _sweep_words(who, words):
    """Threshold words -> contiguous np.uint16 [N]: 1..SWEEP_MAX_THRESHOLDS integers in 1..PROB_ONE, strictly ascending, or ValueError."""
    try:
        w = np.asarray(words.cpu().numpy() if torch.is_tensor(words) else words)       # (not _host_words: a scalar must stay 0-d to be refused)
    except (TypeError, ValueError):
        raise ValueError("%s: words = %r are not integers" % (who, words)) from None
    if w.ndim != 1 or not 1 <= w.size <= SWEEP_MAX_THRESHOLDS or w.dtype.kind not in "iu":
        raise ValueError("%s: words must be 1..%d integers in one dimension, got %s %s" % (who, SWEEP_MAX_THRESHOLDS, w.dtype, w.shape))
    w = w.astype(np.int64)
    if w[0] < 1 or w[-1] > PROB_ONE or (np.diff(w) <= 0).any():
        raise ValueError("%s: words must lie in 1..%d and ascend strictly, got %s" % (who, PROB_ONE, w.tolist()))
    return np.ascontiguousarray(w.astype(np.uint16))


def prob_truth_hist_ws_bytes(nf, H, W, N):
    """pc_prob_truth_hist_ws_bytes (host arithmetic): the bytes of workspace one prob_truth_hist call over nf frames of H x W takes."""
    return _ws_bytes("prob_truth_hist_ws_bytes", "nf = %d frames of %d x %d with N = %d: nf, H, W >= 1, H * W < 2^31, N in 1..%d",
                     nf, H, W, N, tail=(SWEEP_MAX_THRESHOLDS,))


def prob_truth_hist(prob, truth, words, f0=0, nf=None, out=None, ws=None):
    """pc_prob_truth_hist: prob a contiguous 16-bit integer device tensor [F,H,W] (frame_probs': uint16 words), truth contiguous uint8 device
    [F,H,W], words 1..64 host integers in 1..65535, strictly ascending -> out int32 [F, 2, N + 1]: out[f, t, b] the pixels of frame f whose
    truth byte is zero (t = 0) or not (t = 1) and whose probability word has exactly b of the words at or below it, cell [0, 0] included, for
    the frames f0 .. f0 + nf - 1 (default: all from f0 on).  A given out is written in place -- only those frames -- a fresh one is
    zero-filled first.  ws: uint8 device scratch of at least prob_truth_hist_ws_bytes(nf, H, W, N) bytes, made when None."""
    F, H, W = _same_frames("prob_truth_hist", "prob", prob, "truth", truth, _PROB_DTYPES)
    w = _sweep_words("prob_truth_hist", words)
    N = int(w.size)
    f0, nf = _frame_range("prob_truth_hist", F, f0, nf)
    out = _buffer("prob_truth_hist", "out", out, (F, 2, N + 1), torch.int32, prob.device)
    ws = _workspace("prob_truth_hist", ws, prob_truth_hist_ws_bytes(nf, H, W, N), prob.device, "prob_truth_hist_ws_bytes(nf, H, W, N)")
    capi.call("pc_prob_truth_hist", ptr(prob), ptr(truth), F, H, W, f0, nf, w.ctypes.data_as(C.c_void_p), N, ptr(out), ptr(ws), stream())
    return out


def decode_prob_truth_hist(words, N):
    """Host int32 tables of F * 2 * (N + 1) words (numpy or torch, any shape) -> int32 [F, 2, N + 1]."""
    N = int(N)
    return _host_words(words).reshape(-1, 2, N + 1).copy()


def prob_cut_ws_bytes(nf, H, W):
    """pc_prob_cut_ws_bytes (host arithmetic): the bytes of workspace one prob_cut call over nf frames of H x W takes."""
    return _ws_bytes("prob_cut_ws_bytes", "nf = %d frames of %d x %d: nf, H, W >= 1, H * W < 2^31", nf, H, W)


def prob_cut(prob, word, f0=0, nf=None, mask=None, rec=None, ws=None, want_mask=True):
    """pc_prob_cut: prob a contiguous 16-bit integer device tensor [F,H,W] (frame_probs': uint16 words), word an integer in 1..65535 ->
    (mask uint8 [F,H,W] or None, rec int32 [F,8]) for the frames f0 .. f0 + nf - 1 (default: all from f0 on): mask = 1 where the
    probability word is >= word, rec words 0..5 = count, half-open box x0, y0, x1, y1 and the float32 bits of the mean probability word of
    the positive pixels / 65535; words 6 and 7 of a record are left as they are.  Given tensors are written in place -- only those frames --
    fresh ones are zero-filled first.  want_mask=False with mask=None: records only.  ws: uint8 device scratch of at least
    prob_cut_ws_bytes(nf, H, W) bytes, made when None."""
    F, H, W = _frames("prob_cut", "prob", prob, _PROB_DTYPES)
    if not prob.is_cuda:
        raise ValueError("prob_cut: prob must be a device tensor")
    if isinstance(word, (bool, np.bool_)) or not isinstance(word, (int, np.integer)) or not 1 <= int(word) <= PROB_ONE:
        raise ValueError("prob_cut: word = %r is no integer in 1..%d" % (word, PROB_ONE))
    f0, nf = _frame_range("prob_cut", F, f0, nf)
    mask, rec, ws = _detect_buffers("prob_cut", prob.device, F, H, W, mask, rec, ws, want_mask, "prob_cut_ws_bytes(nf, H, W)",
                                    prob_cut_ws_bytes(nf, H, W), any_ws=False)
    capi.call("pc_prob_cut", ptr(prob), F, H, W, f0, nf, int(word), ptr(mask), ptr(rec), ptr(ws), stream())
    return mask, rec


BOX_MAX = 32                               # PC_BOX_MAX of include/picons.h: the rects of one frame
BOX_WORDS = 5                              # PC_BOX_WORDS: a rect is (x0, x1, y0, y1, value), half-open, frame coordinates


def paint_boxes(rects, F, H, W, f0=0, nf=None, binary=False, truth=None):
    """pc_paint_boxes: rects a contiguous int32 device tensor [F,R,5], a row of R rects (x0, x1, y0, y1, value) for every frame of the video ->
    truth uint8 [F,H,W]: in the frames f0 .. f0 + nf - 1 (default: all from f0 on) a pixel holds the low byte of the value of the last rect of
    its frame's row that contains it, 0 if none does -- binary=True: 1 instead of the value.  A rect is intersected with the frame; one with
    x1 <= x0, y1 <= y0 or a zero low byte paints nothing.  A given truth is written in place, in those frames only; a fresh one is as the
    allocator left it where the launch writes all of it (f0 = 0, nf = F) and zero-filled first otherwise."""
    F, H, W = int(F), int(H), int(W)
    if F < 1 or H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError("paint_boxes: F = %d frames of %d x %d: F, H, W >= 1, H * W < 2^31" % (F, H, W))
    _operand("paint_boxes", "rects", rects, torch.int32, dim=3, what="[F,R,5]")
    if not rects.is_cuda:
        raise RuntimeError("picons ops need CUDA/HIP tensors (no CPU fallback)")
    if int(rects.shape[0]) != F or int(rects.shape[2]) != BOX_WORDS:
        raise ValueError("paint_boxes: rects of shape %s, expected (%d, R, %d)" % (tuple(rects.shape), F, BOX_WORDS))
    R = _bound("paint_boxes", "R", rects.shape[1], BOX_MAX)
    f0, nf = _frame_range("paint_boxes", F, f0, nf)
    truth = _buffer("paint_boxes", "truth", truth, (F, H, W), torch.uint8, rects.device, fill=not (f0 == 0 and nf == F))
    capi.call("pc_paint_boxes", ptr(rects), R, F, H, W, f0, nf, int(bool(binary)), ptr(truth), stream())
    return truth


def video_class(scores, out=None):
    """pc_video_class: scores contiguous float32 device [n,C] -> float32 device [C + 2]: mean class scores, arg-max (as a float), its mean."""
    n, C_ = (int(v) for v in _operand("video_class", "scores", scores, torch.float32, dim=2, what="[n,C]").shape)
    out = _buffer("video_class", "out", out, (C_ + 2,), torch.float32, scores.device, fill=False)
    capi.call("pc_video_class", ptr(scores), n, C_, ptr(out), stream())
    return out


def resize_u8(src, Ho, Wo, interpolation, binarize=False):
    """cv2.resize(src, (Wo, Ho), interpolation) on uint8 device images (pc_resize_u8): src [n,H,W,C] or [n,H,W] contiguous;
    interpolation = cv2's flag value (0 nearest, 1 linear, 3 area).  The coordinate / coefficient table is computed on the
    host by the library (pc_resize_tables) and cached on the device per (interpolation, sizes, device)."""
    _operand("resize_u8", "src", src, torch.uint8, dim=(3, 4), what="[n,H,W,C] or [n,H,W]")
    n, H, W = (int(v) for v in src.shape[:3])
    Cc = int(src.shape[3]) if src.dim() == 4 else 1
    tab = _host_table("pc_resize_tables", (int(interpolation), H, W, int(Ho), int(Wo)), src.device)
    dst = torch.empty((n, int(Ho), int(Wo)) + ((Cc,) if src.dim() == 4 else ()), dtype=torch.uint8, device=src.device)
    capi.call("pc_resize_u8", ptr(src), n, H, W, Cc, int(Ho), int(Wo), ptr(tab), int(bool(binarize)), ptr(dst), stream())
    return dst
