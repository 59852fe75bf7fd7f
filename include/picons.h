/* picons.h - C ABI of libpicons.so: the MI355X (gfx950) hot path of the semi-supervised
 * video action-detection train step (AKASH2907/pi-consistency-activity-detection).
 *
 * The reference has NO native/FFI layer: its boundary is the Python module
 * surface.  This ABI sits underneath that surface; each entry cites the reference call site
 * (an ATen op launched from Python) it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers + POD descriptors, no torch types.  All tensor pointers are
 *    DEVICE pointers to fp32 unless stated.  Activations are NDHWC (channels innermost) with
 *    an explicit channel stride `ld*` so a kernel can read/write a channel slice of a wider
 *    tensor (torch.cat becomes free); the pointer passed already includes the channel offset.
 *  - Ownership: the caller owns every buffer incl. workspaces; the library allocates nothing,
 *    keeps no pointers between calls, and only enqueues work on the hipStream_t it is given
 *    (never the null stream implicitly, no device sync).  Entries are re-entrant.
 *  - Errors: int return, 0 = ok, negative = PC_E_*; message via pc_last_error() (thread-local).
 *    Nothing throws across the ABI or calls exit().
 */
#ifndef PICONS_H
#define PICONS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* pc_stream;            /* hipStream_t */

#define PC_OK            0
#define PC_E_ARG        -1          /* bad descriptor / unsupported shape */
#define PC_E_LAUNCH     -2          /* hip launch error */
#define PC_E_NODEVICE   -3

#define PC_ACT_NONE 0
#define PC_ACT_RELU 1
#define PC_ACT_SIGMOID 2

#define PC_F_ACCUM   1              /* out += result (dgrad into a tensor with several consumers) */
#define PC_F_BIAS    2
#define PC_F_CSCALE  4              /* multiply by cscale[n][co] (Dropout3d draw, capsules_ucf101.py:428,507) */
#define PC_F_BNPART  8              /* emit per-block BatchNorm partial sums (sum, sumsq) */
#define PC_F_NFAST   16             /* GEMM rows ordered (t,h,w,n) instead of (n,t,h,w): a 128-row tile is a narrow spatial
                                       patch of all samples, so taps that are padding for the whole tile are skipped
                                       (9x9 ConvTranspose / PrimaryCaps dgrad: 784 gathered vs 400 real positions); with groups the
                                       order holds inside each group */
#define PC_F_TOUT    32             /* channel-major output: out[(n * ldo + co) * (To*Ho*Wo) + position] instead of
                                       out[(n*To*Ho*Wo + position) * ldo + co].  Plain launches only (no bias / activation / cscale /
                                       accumulate / BN partials): the merged tail's column GEMMs, whose gather then streams every
                                       column entry once instead of pulling 4 bytes out of 27 different 512-byte rows */
#define PC_F_CI3     64             /* Ci == 4 whose 4th channel is padding (the RGB clip, 3 channels in 16-byte pieces): that
                                     * channel is taken as zero whatever it holds; the LDS-DMA stem kernel skips its MFMAs */

#define PC_F_STRIPS  256            /* pc_wino_conv, F(2x2, 3x3) only: blocks of two 2 x 14-tile strips taken from pairs of planes (n, n + 1) instead of one
                                     * rectangle of 64 tiles per block -- 56 instead of 49 of a block's 64 tile slots on 28 x 28 frames; needs a tile grid
                                     * a multiple of 14 wide, an even number of tile rows and N % 4 == 0, and is ignored otherwise.  Bit-identical
                                     * results; BatchNorm partial rows then number pc_wino_bnpart_rows(d) for THIS flag setting */
#define PC_F_X6      128            /* the launch multiplies on the bf16 matrix cores: fp32 operands as exact sums of three bf16 values, six
                                     * products, fp32 accumulate (pc_conv_fwd_x6; the caller holds the weights as bf16 planes) */
#define PC_F_BKMAJOR 512            /* with PC_F_X6: the weight planes are K-major, [Ci][KT*KH*KW][ldw] with the OUTPUT channel contiguous (Co <= ldw,
                                     * Co % 8 == 0; group g at + g * wgstride) -- the forward planes of a layer, read as they are by its input
                                     * gradient, so no transposed copy is made.  Same tile, split, work counts and variant string as without
                                     * the flag, bit-identical results; built for the 64 x 128, 128 x 64 and 64 x 64 tiles only (PC_E_ARG otherwise) */

/* ABI version of this header: bumped whenever a struct in it grows or an op's operands change (101: pc_wino_desc.m, PC_OP_BN_FIN_APPLY,
 * pc_wgrad_desc.ws_slices, pc_transpose_job.nslices / slice_stride, pc_wgrad_slices; 102: the workspace operands of PC_OP_TAIL6_WGRAD_MAP / PC_OP_TAIL6_BIAS_SUMS /
 * PC_OP_TAIL_GRADS; 103: the variant reporters pc_conv_variant / pc_wino_variant / pc_wgrad_variant;
 * 104: PC_F_BKMAJOR, pc_wino_weights_multi / PC_OP_WINO_WEIGHTS_MULTI; 105: pc_val_metrics / PC_OP_VAL_METRICS;
 * 106: pc_truth_frame_flags / pc_eval_clips_from_u8 / pc_video_vote;
 * 107: pc_clips_from_u8 / pc_detect_frames / pc_detect_frames_ws_bytes / pc_video_class; the entries pc_clips_from_u8_views / pc_detect_frames_views /
 * pc_detect_frames_views_ws_bytes came later and move nothing: no struct grew, no op's operands changed; so did pc_frame_instances with its
 * PC_INST_* constants, pc_frame_probs / pc_instance_scores with PC_PROB_ONE / PC_SCORE_WORDS, pc_instance_overlaps with PC_LINK_MAX_LAGS, pc_mask_run_ws_bytes /
 * pc_mask_run_index / pc_mask_runs with PC_RUN_WORDS, pc_map_crosstab / pc_map_crosstab_ws_bytes with PC_CROSS_MAX_SLOTS, and pc_resample_tables / pc_detect_frames_scaled_ws_bytes /
 * pc_detect_frames_scaled, and pc_clip_hop_starts / pc_clip_planes_bytes / pc_clip_planes / pc_detect_frames_planes_ws_bytes /
 * pc_detect_frames_planes with PC_PLANES_MAX_FRAMES, and pc_prob_truth_hist_ws_bytes / pc_prob_truth_hist with PC_SWEEP_MAX_THRESHOLDS, and
 * pc_prob_cut_ws_bytes / pc_prob_cut, and pc_paint_boxes with PC_BOX_MAX / PC_BOX_WORDS: came later, move nothing).  Descriptors must be zero-initialised by the caller:
 * fields added later read as "old behaviour" when 0.  pc_version() returns the value the library was built with; the Python host
 * (capi.lib()) refuses a library whose version differs from the header it mirrors. */
#define PC_VERSION 107
int         pc_version(void);
const char* pc_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Generalised gather-GEMM convolution (fp32 MFMA v_mfma_f32_32x32x2_f32, LDS-tiled).
 *   out[n, q*ostr+ooff, co] = act( bias[co] + sum_{a,b,c} sum_ci
 *        in[n, q*istr + ioff0 + (a,b,c)*istep, ci] * w[co][wtap(a,b,c)][ci] ) * cscale[n][co]
 *   wtap = ((wk0_t + a*wkstep_t)*KH + wk0_h + b*wkstep_h)*KW + wk0_w + c*wkstep_w
 * Weight layout [Co][KT*KH*KW][ldw] (taps then channels innermost).  One descriptor covers
 *   nn.Conv3d/Conv2d forward incl. TF-SAME padding folded in (pytorch_i3d.py:112-115; capsules_ucf101.py:44-45,490,497,501),
 *   conv dgrad (stride 1: mirrored taps; stride s: one launch per output-parity class),
 *   nn.ConvTranspose2d/3d forward as sub-pixel parity classes (capsules_ucf101.py:486,495,499,504),
 *   and ConvTranspose dgrad (= strided conv).
 * Requires Ci % 4 == 0, ldi % 4 == 0, ldw % 4 == 0 (float4 loads). */
typedef struct pc_conv_desc {
    int32_t N;
    int32_t Ti, Hi, Wi, Ci, ldi;
    int32_t Tq, Hq, Wq;
    int32_t To, Ho, Wo, Co, ldo;
    int32_t ostr[3], ooff[3];
    int32_t istr[3], ntap[3], ioff0[3], istep[3];
    int32_t wk0[3], wkstep[3];
    int32_t KT, KH, KW, ldw;
    int32_t act, flags;
    int32_t wgstride, bgstride;     /* per-group weight / bias offsets (floats): group g uses w + g*wgstride, bias + g*bgstride
                                       (per-sample collapsed decoder-tail weights); 0 = shared */
    int32_t act_c0;                 /* activation applies to output channels >= act_c0 (merged pose|activation conv) */
    int32_t groups;                 /* >=1: rows are tiled per batch group (N/groups samples each) so BatchNorm
                                       partials never straddle the two forward passes of one step */
} pc_conv_desc;

/* bnpart: [pc_conv_bnpart_rows(d)][2][Co] partial (sum, sumsq) over output rows, or NULL.
 * Size limit: the LDS-DMA gather addresses `in` and `w` with 32-bit byte offsets from a wave-uniform base, so each must be smaller than
 * 4 GiB (0xff000000 bytes; PC_E_ARG otherwise -- the largest activation at bs = 8 is 0.8 GB).  Same for D / S of pc_conv_wgrad and for one
 * (H, W, ldi) frame of pc_wino_conv. */
int pc_conv_fwd(const pc_conv_desc* d, const float* in, const float* w, const float* bias,
                const float* cscale, float* out, float* bnpart, pc_stream s);
int pc_conv_bnpart_rows(const pc_conv_desc* d);

/* The same convolution with the fp32 multiplications carried out on the bf16 matrix cores (csrc/conv_x6.hip): every fp32 operand is split
 * exactly into three bf16 values h + m + l and the six products of weight >= 2^-16 are accumulated in fp32 -- closer to an fp64 result than
 * an fp32 FMA chain (tests/test_x6_gpu.py), 1.5 - 1.8x the rate of v_mfma_f32_32x32x2_f32.  `in` stays fp32 (split in registers); the weights
 * come as three bf16 planes, each in the layout of `w` above ([Co][KT*KH*KW][ldw], group g at + g * wgstride elements), plane p at
 * wplanes + p * plane_stride elements -- pc_split_planes makes them from the fp32 layout.  d->flags must carry PC_F_X6 and
 * pc_conv_x6_ok(d) must hold (Ci % 32 == 0, ldw % 8 == 0, <= 10 taps per dimension); everything else as pc_conv_fwd. */
int pc_conv_fwd_x6(const pc_conv_desc* d, const float* in, const uint16_t* wplanes, int64_t plane_stride, const float* bias,
                   const float* cscale, float* out, float* bnpart, pc_stream s);
/* With a workspace the launch may split the tiles of its last, partly filled round of resident blocks (or all tiles, when it does not fill
 * one round) into K slices: one block per slice leaves its partial sums in `ws`, the last block to arrive at a tile adds them in slice order
 * and runs the epilogue -- same results whichever block that is (run-to-run bit-identical), every epilogue supported.  pc_conv_x6_ws_floats(d)
 * = floats the launch wants (0: it would not split).  The LAST ceil(rem / 4) * 4 floats of that size are per-tile counters: they must be ZERO
 * before the first launch that uses the workspace, every launch leaves them zero.  ws == NULL: pc_conv_fwd_x6. */
int64_t pc_conv_x6_ws_floats(const pc_conv_desc* d);
int pc_conv_fwd_x6_ws(const pc_conv_desc* d, const float* in, const uint16_t* wplanes, int64_t plane_stride, const float* bias,
                      const float* cscale, float* out, float* bnpart, float* ws, int64_t ws_floats, pc_stream s);
int pc_conv_x6_ok(const pc_conv_desc* d);       /* host-only advice for a planner: 1 if the descriptor (with PC_F_X6) can take the bf16-split kernel AND is
                                                  * large enough to gain from it (small launches are faster on pc_conv_fwd) */
/* planes[p * plane_stride + i] = p-th bf16 term of src[i] (p = 0, 1, 2: h = bf16(x), m = bf16(x - h), l = x - h - m, round to nearest; h + m + l == src[i] exactly for 2^-110 <= |x| < 2^128);
 * n and plane_stride multiples of 4 */
int pc_split_planes(const float* src, uint16_t* planes, int64_t n, int64_t plane_stride, pc_stream s);
/* the same for many buffers in one launch (the per-step weight planes); `jobs` is HOST memory */
typedef struct pc_split_job {
    uint64_t src, planes;           /* device pointers */
    int64_t  n, plane_stride;
} pc_split_job;
int pc_split_planes_multi(const pc_split_job* jobs, int njobs, pc_stream s);
/* Host-only work accounting of one pc_conv_fwd launch (no GPU call; measurement support for bench.py / tools/launch_table.py,
 * no reference counterpart).  Walks the launch's tiles in the kernel's own row order and counts the K loop each block really
 * runs (taps that are padding for every row of a tile are skipped by the kernel).  out[7]:
 *   [0] multiply-accumulates ISSUED to the matrix cores (whole tiles: what an MFMA instruction counter sees),
 *   [1] EXECUTED on real outputs (real rows x real columns x the tile's K; padding taps inside the tile's tap box included),
 *   [2] VALID (taps that read inside the volume, real channels only),  [3] blocks,  [4] BM,  [5] BN,
 *   [6] 1 = LDS-DMA kernel with the per-tile tap box, 0 = register-staged kernel (flattened K).
 * ci_real / co_real: channels that are not padding (0 = Ci / Co). */
int pc_conv_work(const pc_conv_desc* d, int ci_real, int co_real, double* out);
/* Host-only (no GPU call): the kernel template instance pc_conv_fwd -- for a PC_F_X6 descriptor pc_conv_fwd_x6_ws with a workspace of ws_floats
 * floats (0 = none) -- WOULD launch for this descriptor with 16-byte aligned operands, as one NUL-terminated string in buf[cap].  It comes from
 * the decision code the launch itself runs, so tests can say which variant a case exercises (tests/variant_cases.py):
 *   conv:<glds|glds_tap8|reg_fast|reg_ragged>:<BM>x<BN>:w<WM>x<WN>[:st<LDS-DMA ring depth>][:ci3]
 *        glds = LDS-DMA gather, glds_tap8 = its 8-taps-per-chunk form for Ci == 4, reg_* = register-staged gather with K a multiple of 32 / ragged
 *   x6:<BM>x<BN>:w<WM>x<WN>:ks<K slices of the tail tiles; 1 = no tail split>[:mfast]        mfast = row tiles fastest in the block order */
int pc_conv_variant(const pc_conv_desc* d, int64_t ws_floats, char* buf, int cap);

/* ------------------------------------------------------------------------------------------
 * Winograd F(2x2, 3x3) form of the stride-1, "same"-padded KT x 3 x 3 convolutions (KT = 3 with temporal padding 1, or 1):
 *   out[n,t,h,w,co] = act( bias[co] + sum_{kt,kh,kw,ci} in[n, t+kt-KT/2, h+kh-1, w+kw-1, ci] * g[co][kt][kh][kw][ci] )   (zero padding)
 * 2.25x fewer multiply-accumulates than pc_conv_fwd for the same result (equal in exact arithmetic; fp32 rounding differs at the
 * 1e-6 level).  Used for the decoder's skip convs and Conv3d_2c and for their input gradients (nn.Conv3d forward / ATen
 * convolution_backward's input branch: capsules_ucf101.py:497,501; pytorch_i3d.py:236-238).  H, W even; Ci % 8 == 0.
 * The weights are passed in the transform domain: pc_wino_weights builds U (pc_wino_u_floats(O, I, KT) floats) from any strided
 * weight tensor w[o*sO + ((kt*3+kh)*3+kw)*sT + i*sI] -- the master OIDHW tensor directly (sO = I*KT*9, sT = 1, sI = KT*9), or, with
 * flip = 1 and O / I exchanged (sO = KT*9, sI = Cout*KT*9), the mirrored / transposed weights of the input gradient.
 * flags: PC_F_BIAS, PC_F_ACCUM, PC_F_BNPART (partials [pc_wino_bnpart_rows(d)][2][Co]; rows of one sample are consecutive, samples
 * in order, so the rows of a batch group are one contiguous range). */
typedef struct pc_wino_desc {
    int32_t N, T, H, W;             /* output frames / positions (H, W: stride 1, same padding, so input = output size) */
    int32_t Ci, ldi, Co, ldo;
    int32_t KT;                     /* temporal taps: 3 or 1 */
    int32_t act, flags;             /* PC_ACT_NONE / PC_ACT_RELU */
    int32_t Ti;                     /* input frames */
    int32_t ta, tc, tden;           /* tap kt of output frame t reads input frame (t*ta + kt + tc) / tden when that is an integer in
                                     * [0, Ti): forward with temporal stride s and front padding p: (s, -p, 1); input gradient of that
                                     * layer (weights mirrored): (1, p - (KT-1), s).  Stride 1, padding KT/2: (1, -(KT/2), 1) both ways */
    int32_t m;                      /* output tile edge: 2 (or 0) = F(2x2, 3x3); 4 = F(4x4, 3x3): 4x fewer multiply-accumulates than the direct
                                     * form for ~3x the rounding error of F(2x2, 3x3); H, W multiples of 4, Ci % 8 == 0, and U
                                     * from pc_wino4_weights (pc_wino4_u_floats floats) */
} pc_wino_desc;
int64_t pc_wino_u_floats(int O, int I, int KT);
int pc_wino_weights(const float* w, int64_t sO, int64_t sT, int64_t sI, int O, int I, int KT, int flip, float* U, pc_stream s);
int pc_wino_conv(const pc_wino_desc* d, const float* in, const float* U, const float* bias, float* out, float* bnpart, pc_stream s);
/* transform-domain weights of the m = 4 form (same addressing of w as pc_wino_weights) */
int64_t pc_wino4_u_floats(int O, int I, int KT);
int pc_wino4_weights(const float* w, int64_t sO, int64_t sT, int64_t sI, int O, int I, int KT, int flip, float* U, pc_stream s);
/* many weight transforms of either form in ONE launch (the per-step transforms of the layers whose prep runs on one lane); `jobs` is HOST memory.
 * Each job is one pc_wino_weights (m = 2 or 0) / pc_wino4_weights (m = 4) call: same arithmetic, bit-identical U. */
typedef struct pc_wino_weights_job {
    uint64_t w, U;                  /* device pointers */
    int64_t  sO, sT, sI;
    int32_t  O, I, KT, flip, m, reserved;
} pc_wino_weights_job;
int pc_wino_weights_multi(const pc_wino_weights_job* jobs, int njobs, pc_stream s);
int pc_wino_bnpart_rows(const pc_wino_desc* d);
/* host-only work accounting (see pc_conv_work): out[0] issued, out[1] executed multiply-accumulates, out[2] blocks */
int pc_wino_work(const pc_wino_desc* d, double* out);
/* host-only, as pc_conv_variant: wino2:<BTH>x<BTW>|strips:<vec|scalar> or wino4:<BTH>x<BTW>:<vec|scalar> -- F(2x2) / F(4x4), the tile rectangle of a
 * block (or strip mode), 16-byte or four-byte stores in the epilogue.  Of `out` only the alignment counts (NULL = 16-byte aligned). */
int pc_wino_variant(const pc_wino_desc* d, const float* out, char* buf, int cap);

/* Weight gradient:  g[m][ (a,b,c) , cs ] += sum_{n,q} D[n,q,m] * S[n, q*istr+ioff0+(a,b,c)*istep, cs]
 * D dense over the lattice (Tq,Hq,Wq), S gathered.  g layout [Cd][KT*KH*KW][Cs], tap (a,b,c) -> wk0+(a,b,c),
 * accumulated with fp32 atomics (g must be initialised).  Conv3d wgrad: D=dY, S=X;
 * ConvTranspose wgrad: D=X, S=dOut.  (replaces ATen convolution_backward's weight branch.) */
typedef struct pc_wgrad_desc {
    int32_t N;
    int32_t Tq, Hq, Wq, Cd, ldd;
    int32_t Ts, Hs, Ws, Cs, lds;
    int32_t istr[3], ntap[3], ioff0[3], istep[3];
    int32_t wk0[3];                 /* first weight tap per dim (taps that only ever see padding are trimmed by the host) */
    int32_t KT, KH, KW;             /* full weight tap extents: g is [Cd][KT*KH*KW][Cs] */
    int32_t splitk;                 /* 0 = choose; -1 = one slice written with plain stores (g need not be initialised;
                                     * only valid when no tap is trimmed: ntap == (KT,KH,KW)) */
    int32_t nbatch;                 /* 0/1 = one problem; > 1: that many independent problems in ONE launch (blockIdx.z =
                                     * problem * slices + slice), D, S and g advanced by the strides below (floats) */
    int32_t dbstride, sbstride, gbstride;
    int32_t Td, Hd, Wd, doff[3];    /* Td > 0: D is not dense but the sub-lattice (Tq,Hq,Wq) starting at doff of a
                                     * [N][Td][Hd][Wd][ldd] tensor (with nbatch > 1: per problem, N = 1 each) */
    int32_t flags;                  /* PC_WG_CS3: Cs == 4 whose 4th channel is padding -- g[..][3] may be left untouched */
    int32_t ws_slices;              /* 0: K slices are combined with fp32 atomics in g (arrival order).  n > 0: g is a WORKSPACE of n images of the
                                     * gradient, each Cd*KT*KH*KW*Cs floats (nbatch > 1: gbstride*nbatch) -- slice k leaves its partial sums in image k
                                     * with plain stores, n >= pc_wgrad_slices(d); the consumer adds the images in slice order
                                     * (pc_transpose_job.nslices), so the gradient is bit-identical from run to run.  The workspace must be
                                     * zero before its FIRST use (trimmed taps and empty slices are never written) and needs no fill after. */
} pc_wgrad_desc;
#define PC_WG_CS3    1
#define PC_WG_X6     2              /* the row-segment (3 taps along w, padding 1), generic split-K and -- together with PC_WG_CS3 -- stem kernels multiply
                                     * on the bf16 matrix cores: both operands split into three bf16 terms in registers, six products, fp32
                                     * accumulate (as pc_conv_fwd_x6); the 9-tap spectral route ignores it (pc_wgrad_uses_x6) */
int pc_conv_wgrad(const pc_wgrad_desc* d, const float* D, const float* S, float* g, pc_stream s);
/* K slices the launch(es) of pc_conv_wgrad make for this problem (host-only, no GPU call; ws_slices is ignored): the number of workspace
 * images a caller that sets ws_slices has to provide.  -1 on a bad descriptor. */
int pc_wgrad_slices(const pc_wgrad_desc* d);
/* host-only, as pc_conv_variant (a dry run of pc_conv_wgrad): <kernel><template arguments>[+<second launch>]:k<K slices>:<store|atomic|ws> with
 * wgrad4[_x6] the 7 x 7 stem, wgrad3[_x6]<BM,BKP,CSB,WMW[,KW]> the row-segment kernels, wgrad[_x6]<BM,BN[,positions per chunk]> generic split-K;
 * store = plain stores of one slice (splitk = -1), atomic = fp32 atomics, ws = ordered K-slice images (ws_slices > 0). */
int pc_wgrad_variant(const pc_wgrad_desc* d, char* buf, int cap);
/* Folds the K-slice images of a workspace in place, for launches with many slices: image g*G of every group of G = pc_wgrad_fold_group()
 * consecutive images becomes the sum of its group (slice order); the consumer then adds ceil(nslices / G) images G*image_floats apart. */
int pc_wgrad_fold_group(void);
int pc_wgrad_fold(float* ws, int64_t image_floats, int nslices, pc_stream s);
/* Host-only work accounting of one pc_conv_wgrad launch (no GPU call; see pc_conv_work).  out[5]: multiply-accumulates ISSUED to
 * the matrix cores, EXECUTED on real rows x columns, VALID (non-padding source positions), and the kernel family the problem is
 * routed to (0 stem, 1 row-segment with 3 taps, 2 row-segment with 9 taps, 3 generic split-K), kernel launches the call makes.
 * cd_real / cs_real: 0 = Cd / Cs. */
int pc_wgrad_work(const pc_wgrad_desc* d, int cd_real, int cs_real, double* out);
/* 1 if the problem's launch multiplies on the bf16 matrix cores (PC_WG_X6 on the row-segment, generic and -- with PC_WG_CS3 -- stem routes), 0 if on
 * fp32 MFMA (host-only; bench.py's two weight-gradient roofline legs and pc_run_ops_timed's sub-filter split the family by it) */
int pc_wgrad_uses_x6(const pc_wgrad_desc* d);
/* Several weight gradients in one call (the wgrads of one Inception module; the eight position classes of the merged tail):
 * the problems the generic split-K kernel would take share ONE grid, each with a range of blocks in proportion to its work; the
 * others (stem, row-segment, long-K shapes) get their usual launch.  Same results as njobs pc_conv_wgrad calls up to the order
 * of the fp32 atomic sums.  `jobs` is host memory. */
typedef struct pc_wgrad_job {
    pc_wgrad_desc d;
    const float* D; const float* S; float* g;
} pc_wgrad_job;
int pc_conv_wgrad_multi(const pc_wgrad_job* jobs, int njobs, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * BatchNorm3d(train) + ReLU (pytorch_i3d.py:116-119; eps 1e-3, momentum 0.01 at :80).
 * `groups`: the two forward passes of one step (main_ucf101.py:85-86) run as one batch whose
 * rows split into `groups` equal row ranges with separate batch statistics; running stats
 * are updated once per group, in order (as the reference's two sequential forwards do). */
/* partials [groups][nparts_per_group][2][C] (sum, sumsq from pc_conv_fwd) -> stat[groups][4][C] =
 * mean, invstd, scale=gamma*invstd, shift=beta-mean*scale; running stats updated if non-NULL. */
int pc_bn_finalize(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group,
                   const float* gamma, const float* beta, float eps, float momentum,
                   float* running_mean, float* running_var, float* stat, pc_stream s);
/* The same with a workspace of pc_bn_finalize_ws_floats(...) floats (0 for fewer than 512 partial rows per group): layers with
 * thousands of partial rows (the stem: 2 x 6272) are reduced in two stages -- 32 blocks per 16 channels and group, then the finalize
 * over their double-precision partial rows -- instead of by one block per 16 channels (85 -> 15 us on the dependency chain).  ws NULL
 * = the one-stage form.  Fixed summation order either way. */
int64_t pc_bn_finalize_ws_floats(int nparts_per_group, int groups, int C);
int pc_bn_finalize_ws(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group,
                      const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, float* stat, float* ws, pc_stream s);
/* y[r][c] = relu?(z[r][c]*scale[g(r)][c]+shift[g(r)][c]) */
int pc_bn_apply(const float* z, int ldz, const float* stat, int C, int64_t rows, int groups, float* y,
                int ldy, int relu, pc_stream s);
/* eval mode: stat[4][C] from running stats */
/* pc_bn_finalize + pc_bn_apply in ONE launch, for layers with at most 256 partial rows per batch group (pc_bn_finalize_apply_ok): every block
 * of the apply kernel reduces the partial rows of its own 64 channels (doubles, fixed order) and streams its rows; row block 0 of group 0 writes
 * `stat` and the running statistics (groups in order).  Round 5: one dispatch fewer per BatchNorm site on the step's dependency chain
 * (/root/reference/models/pytorch_i3d.py:116-119).  Arguments as the two calls it replaces; rows = all rows of z (every group). */
int pc_bn_finalize_apply_ok(int nparts_per_group, int C);
int pc_bn_finalize_apply(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group, const float* gamma, const float* beta,
                         float eps, float momentum, float* running_mean, float* running_var, float* stat, const float* z, int ldz, int64_t rows,
                         float* y, int ldy, int relu, pc_stream s);
int pc_bn_eval_stat(const float* gamma, const float* beta, const float* running_mean,
                    const float* running_var, float eps, int C, float* stat, pc_stream s);
/* backward: dy (grad after ReLU, row stride lddy), z -> dz; dgamma/dbeta (+)= if accum.
 * ws: >= pc_bn_bwd_ws_floats(rows,C,groups) floats.  relu: bit 0 = the layer has a ReLU; bit 1 = the finalize folded into the apply kernel
 * (two launches instead of three; measured: no gain, the planner never sets it by itself -- switches.py PICONS_BN_FUSED). */
int64_t pc_bn_bwd_ws_floats(int64_t rows, int C, int groups);
int pc_bn_bwd(const float* dy, int lddy, const float* z, int ldz, const float* stat, int C,
              int64_t rows, int groups, int relu, float* dz, int lddz, float* dgamma, float* dbeta,
              int accum, float* ws, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * MaxPool3d with TF-SAME zero padding (pytorch_i3d.py:21-45); argmax kept for the backward. */
typedef struct pc_pool_desc {
    int32_t N, Ti, Hi, Wi, C, ldi;
    int32_t To, Ho, Wo, ldo;
    int32_t k[3], s[3], padf[3];
} pc_pool_desc;
int pc_maxpool_fwd(const pc_pool_desc* d, const float* x, float* y, uint8_t* argmax, pc_stream s);
int pc_maxpool_bwd(const pc_pool_desc* d, const float* dy, const uint8_t* argmax, float* dx,
                   int accum, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Elementwise helpers */
/* y[n,pos,c] = x[n,pos,c] * scale[n][c]  (Dropout3d, capsules_ucf101.py:428; also its backward) */
int pc_channel_scale(const float* x, int ldx, const float* scale, int N, int64_t pos_per_n, int C,
                     float* y, int ldy, int accum, pc_stream s);
/* dz = dy * act'(y) ; dbias[c] (+)= sum dz   (bias+ReLU / bias+sigmoid / bias-only epilogues) */
int64_t pc_act_bwd_ws_floats(int64_t rows, int C);
int pc_act_bwd(const float* dy, int lddy, const float* y, int ldy, int act, int C, int64_t rows,
               float* dz, int lddz, float* dbias, int accum, float* ws, pc_stream s);
/* NCDHW (reference layout, main_ucf101.py:52-59 input clips) -> NDHWC with C padded to Cpad;
 * flipw mirrors W (torch.flip(.,[4]), main_ucf101.py:100). src may be fp32 or fp64. */
int pc_ncdhw_to_ndhwc(const void* src, int src_is_f64, int N, int C, int64_t thw, int W, int Cpad,
                      int flipw, float* dst, pc_stream s);
int pc_ndhwc_to_ncdhw(const float* src, int ld, int N, int C, int64_t thw, float* dst, pc_stream s);
/* dst[b][c][r] (+)= src[b][r][c] through 32x32 LDS tiles.  Every weight / weight-gradient
 * re-layout between the reference's OI(T)HW / IO(T)HW state_dict layout and the kernels'
 * [O][taps][I] / [I][taps][O] layouts is one call of this (see plan.py). */
int pc_transpose_batched(const float* src, int batch, int R, int Cc, int64_t src_batch_stride,
                         int src_ld, float* dst, int64_t dst_batch_stride, int dst_ld, int accum,
                         pc_stream s);
/* the same for many independent jobs in one launch (the per-step weight re-layouts); `jobs` is HOST memory */
typedef struct pc_transpose_job {
    uint64_t src, dst;              /* device pointers */
    int64_t  src_batch_stride, dst_batch_stride;
    int32_t  batch, R, C, src_ld, dst_ld, accum;
    int32_t  nslices, reserved;     /* nslices > 1: src is that many images slice_stride floats apart (the K-slice images of a weight gradient,
                                     * pc_wgrad_desc.ws_slices); they are added in slice order on the way -- dst (+)= sum_k src_k^T */
    int64_t  slice_stride;
} pc_transpose_job;
int pc_transpose_multi(const pc_transpose_job* jobs, int njobs, pc_stream s);
/* dx[n,h,w,c] (+)= sum over valid taps of cols[n, h-b, w-c'][(b*KW+c')*C + c]: gather half of an exact stride-1 'full'
 * correlation (PrimaryCaps dgrad, capsules_ucf101.py:44-45 backward) computed as GEMM + col2im, so only the
 * Ho*Wo real output positions are multiplied instead of the (Ho+KH-1)*(Wo+KW-1) gathered ones. */
int pc_col2im(const float* cols, int N, int Ho, int Wo, int KH, int KW, int C, float* dx, int lddx,
              int accum, pc_stream s);
/* ------------------------------------------------------------------------------------------
 * Evaluation metrics (evaluate_ucf101.py:142-183, evaluate_jhmdb.py same lines): what the reference does in numpy after
 * `segmentation.cpu()`.  pc_seg_frame_counts: per frame of `nframes` x `pix` logits (B,1,8,H,W contiguous = frame-major)
 * and truth masks, counts[frame] = { #(pred+gt == 2), #(pred+gt != 0), #(gt != 0) } with pred = sigmoid(logit) >= 0.5
 * (:128,:148-149,:160-161); the call zeroes `counts` itself.  pc_map_accumulate: one video -- frames with truth add to
 * n_frames[label] and, for every threshold k/20 (float32, :72) that the frame's inter/union (float64) reaches, to
 * frame_hits[label][k]; the video's summed counts do the same for video_hits; n_vids[label] += 1 (:153-183).
 * All tables int32, [ncls][20] / [ncls], owned and zero-initialised by the caller. */
int pc_seg_frame_counts(const float* logits, const float* gt, int64_t nframes, int64_t pix, int32_t* counts, pc_stream s);
int pc_map_accumulate(const int32_t* counts, int64_t nframes, int label, int ncls, int32_t* frame_hits, int32_t* video_hits,
                      int32_t* n_frames, int32_t* n_vids, pc_stream s);
/* Validation pass (main_ucf101.py:33-47 val_model_interface and the loop body of validate :241-264) on one batch: `output` [B][pix]
 * logits and `loc_msk` [B][pix] truth (fp32, values in {0, 1}; pix = 8*H*W, a multiple of 4, both 16-byte aligned),
 * `predicted_action` [B][C], `action` [B] (int32 class ids).  One record of pc_val_record_words(B) = 10 + 3*B 32-bit words:
 *   float  [0] total = loc + cls   [1] loc = bce + dice   [2] cls   [3] abs_cls   (SpreadLoss over all B rows, utils/losses.py:14-37, margin 0.2)
 *          [4] bce = mean of max(x,0) - x*y + log1p(exp(-|x|))   [5] dice = 1 - (2*sum(s*y) + 1) / (sum(s) + sum(y) + 1), s = sigmoid(x)
 *          [6] sum of inter/union over the clips with gt > 0   [7] their number
 *   int32  [8] n_correct: rows whose arg-max (first maximum) equals action   [9] B
 *          [10 + 3*b ..] per clip: inter = #(x > 0 and y != 0), union = #(x > 0 or y != 0), gt = #(y != 0) -- the sums IOU2 takes
 *          (utils/metrics.py:171-193) for the mask `output > 0` (strict, validate :255; NOT the sigmoid(x) >= 0.5 of pc_seg_frame_counts).
 * Per-element terms are fp32, sums double; block partials go to `ws` (pc_val_metrics_ws_floats(B, pix) floats, 16-byte aligned, contents
 * irrelevant before the call) and are added in block order: no floating-point atomics, the record is bit-identical from run to run.  A row
 * whose action is outside [0, C) makes cls / abs_cls / total NaN and is not counted as correct.  The two size functions are host-only and
 * return -1 for a B or pix the call would refuse. */
int     pc_val_record_words(int B);
int64_t pc_val_metrics_ws_floats(int B, int64_t pix);
int     pc_val_metrics(const float* output, const float* loc_msk, const float* predicted_action, const int32_t* action, int B, int64_t pix,
                       int C, int32_t* record, float* ws, pc_stream s);
/* ------------------------------------------------------------------------------------------
 * Input pipeline (datasets/ucf_dataloader.py:146-173 and the box rasterisation of load_video :204-221): from the decoded
 * uint8 frames `video` [F][H][W][3] in HBM, the 8 frames `span8` (host array), the S x S crop at (h0, w0): data =
 * frame / 255 (float64 division, then float32) as NCDHW [3][8][S][S], aug = its horizontal flip, mask [8][S][S] = 1 where
 * any of the frame's R boxes rects[t][r] = (x0, x1, y0, y1) (device int32, frame coordinates, half-open, already clipped
 * the way numpy clips `bbox[f, y:y+h, x:x+w]`) covers the pixel, else 0. */
int pc_clip_from_u8(const uint8_t* video, int F, int H, int W, const int32_t* span8, int h0, int w0, int S,
                    const int32_t* rects, int R, float* data, float* aug, float* mask, pc_stream s);
/* JHMDB form (datasets/jhmdb_dataloader.py:167-205): the truth is a per-pixel mask per frame, `maskframes` [F][H][W] uint8
 * (> 0 = foreground), and only the frames flagged in valid8 (host array; :187-194) carry it: mask = valid && maskframe > 0,
 * mask_cls [8][S][S] = valid. */
int pc_clip_from_u8_masks(const uint8_t* video, int F, int H, int W, const int32_t* span8, int h0, int w0, int S,
                          const uint8_t* maskframes, const int32_t* valid8, float* data, float* aug, float* mask, float* mask_cls,
                          pc_stream s);
/* pc_clip_from_u8 with data / aug written as [8][S][S][4] float32 (r, g, b, 0) -- the NDHWC layout with the RGB clip padded to one 16-byte piece per
 * position that the network's first conv reads (Conv3d_1a_7x7, PC_F_CI3) -- so that a sample written into its place of the next step's minibatch
 * needs no layout conversion at all (StepEngine.sample_stager); mask as pc_clip_from_u8.  data / aug 16-byte aligned. */
int pc_clip_from_u8_ndhwc4(const uint8_t* video, int F, int H, int W, const int32_t* span8, int h0, int w0, int S,
                           const int32_t* rects, int R, float* data, float* aug, float* mask, pc_stream s);
/* Evaluation input (evaluate_ucf101.py:79-101, :139-146) from one decoded video in HBM: `video` uint8 [F][H][W][3], `truth` uint8 [F][H][W], the
 * S x S crop at (h0, w0) (the eval loader's centre crop, datasets/ucf_dataloader_eval.py:100-106).
 * pc_truth_frame_flags: flags[f] (int32) = number of non-zero truth pixels of frame f inside the crop; one block per frame, a plain store (no
 * atomics, `flags` need not be zeroed).  A clip is kept if one of its in-range frames has a non-zero flag (:95-96).
 * pc_eval_clips_from_u8: `starts` is a HOST array of n first-frame indices (1 <= n <= 32, each >= 0); frame k of clip c is starts[c] + k * f_skip.
 * data [n][8][S][S][4] float32 = (r, g, b, 0) with every channel (float)((double)u8 / 255.0) -- the NDHWC tensor the network's first conv reads
 * (PC_F_CI3), as pc_clip_from_u8_ndhwc4 writes it; gt [n][8][S][S] float32 = the truth VALUE (not binarised), frame-major as pc_seg_frame_counts
 * takes it.  A frame index >= F gives zeros in both and reads nothing (:89-91).  data / gt 16-byte aligned.
 * pc_video_vote: pred [n][C] float32; the n rows are added in row order in fp32 and divided by (float)n (numpy's mean over axis 0 of a C-contiguous
 * float32 array), and *n_correct += 1 if the first maximum is `label` (a NaN mean counts as the maximum, as in np.argmax).
 * All three refuse bad arguments with PC_E_ARG before any HIP call. */
int pc_truth_frame_flags(const uint8_t* truth, int F, int H, int W, int h0, int w0, int S, int32_t* flags, pc_stream s);
int pc_eval_clips_from_u8(const uint8_t* video, const uint8_t* truth, int F, int H, int W, int h0, int w0, int S,
                          const int32_t* starts, int n, int f_skip, float* data, float* gt, pc_stream s);
int pc_video_vote(const float* pred, int n, int C, int label, int32_t* n_correct, pc_stream s);
/* Detection output (csrc/detect.hip; picons_amd/detect.py): unlabelled video in, per-frame masks, boxes and scores and the video's class out.
 * pc_clips_from_u8: pc_eval_clips_from_u8 without the truth side -- the same kernel, the truth a compile-time switch -- writing `data` with the
 * same bits; same refusals.
 * pc_detect_frames: `logits` float32 [n][8][S][S], the eval forward's output for n <= 32 clips of ONE video (16-byte aligned, S % 4 == 0), and
 * the starts / f_skip / F / H / W / h0 / w0 / S the clips were cut with.  Frame k of clip c is video frame f = starts[c] + k * f_skip; for
 * f >= F nothing is read and nothing written.  For f < F the launch writes the WHOLE frame mask[f] of `mask` uint8 [F][H][W] (video frame
 * order, full-frame coordinates): 1 where the pixel lies inside the crop and fp32 sigmoid(x) >= 0.5 -- pc_seg_frame_counts' predicate, one
 * device function for both; NaN is background -- and 0 everywhere else, the margin around the crop included: no fill in front of the launch,
 * and a frame the launch does not address is not touched.  `mask` may be null: records only.  rec int32 [F][8], one record per frame:
 *   [0] count of positive pixels   [1..4] x0, y0, x1, y1, the half-open box of the positive pixels in full-frame coordinates (mask[f, y0:y1,
 *   x0:x1] holds all of them), all zero when count == 0   [5] the bits of the float32 frame score: the mean of the fp32 1 / (1 + expf(-x))
 *   over the positive pixels, summed in double in a fixed order, divided once in double and rounded once; 0.0f when count == 0
 *   [6] row0 + c, the clip row the frame came from   [7] 0
 * No atomics: every block leaves a partial in `ws` (pc_detect_frames_ws_bytes(n, S) bytes, 8-byte aligned, contents irrelevant before the
 * call; host-only, -1 for an n or S the call would refuse) and a second small launch adds them in block order, so a record is bit-identical
 * from run to run.  The starts of one launch must address distinct frames.
 * pc_video_class: scores float32 [n][C] -> out float32 [C + 2]: the mean class scores with pc_video_vote's arithmetic (rows added in row
 * order in fp32, one division by (float)n), then the arg-max as a float (the first maximum; a NaN beats every number), then the mean at it.
 * All refuse bad arguments with PC_E_ARG before any HIP call, allocate nothing and enqueue on `s` only. */
int     pc_clips_from_u8(const uint8_t* video, int F, int H, int W, int h0, int w0, int S, const int32_t* starts, int n, int f_skip,
                         float* data, pc_stream s);
int64_t pc_detect_frames_ws_bytes(int n, int S);
int     pc_detect_frames(const float* logits, int F, int H, int W, int h0, int w0, int S, const int32_t* starts, int n, int f_skip,
                         int row0, uint8_t* mask, int32_t* rec, void* ws, pc_stream s);
int     pc_video_class(const float* scores, int n, int C, float* out, pc_stream s);
/* Multi-view detection (picons_amd/detect.py: DetectEngine(tile=, flip=, views=)).  A view is a crop of the frame, optionally mirrored left-right:
 * `views` is a HOST table int32 [V][3] = h0, w0, flip (1 <= V <= 32, every crop inside the frame, flip 0 or 1).  View v of clip c lies at clip
 * slot v * view_stride + c of `data` / `logits` (view_stride >= n, in clips): the caller decides the slot layout.
 * pc_clips_from_u8_views: pc_clips_from_u8 for all V views of the n <= 32 clips in ONE launch (grid.y = V * n * 8).  An unflipped view holds the
 * bytes pc_clips_from_u8 writes for its crop (the same u8 / 255 table, zeros for a frame index >= F, a fourth channel of exactly 0); in a
 * flipped view data[y][x] is the pixel at (h0 + y, w0 + S - 1 - x).  Slots between the views (view_stride > n) are not touched.
 * pc_detect_frames_views: pc_detect_frames with the views merged per FULL-FRAME pixel in front of the predicate.  The views that cover the pixel
 * are visited in table order (a flipped view is read at x' = S - 1 - (x - w0)): the first value is taken as it is, later ones are added with
 * __fadd_rn, and the sum is divided once with __fdiv_rn by (float)count when count > 1 -- no zero start, so -0.0 and NaN pass through.  A pixel
 * no view covers is background (0).  Mask, predicate (seg_positive), record layout, frame rules (f >= F neither read nor written, a frame the
 * launch does not address untouched, a null `mask` gives records only) and the score's arithmetic (fp32 sigmoid of the MERGED logit, summed in
 * double in a fixed order: thread, wave, block partial in `ws`, a second launch adds the partials in block order) are pc_detect_frames'; the box
 * is in full-frame coordinates and rec[6] = row0 + c * V, the ring row of the clip's first view.  The blocks of a frame stride over its H * W
 * pixels: pc_detect_frames_views_ws_bytes(n, H, W) = n * 8 * min(64, ceil(ceil(H * W / 4) / 1024)) * 32 bytes (host-only; -1 for n outside
 * 1..32, H or W < 1, H * W >= 2^31).  No atomics, nothing to zero in front of the launch.  Refusals: pc_detect_frames' list (S % 4 == 0 and the
 * alignments included), the view-table checks and view_stride < n -- PC_E_ARG before any HIP call. */
int     pc_clips_from_u8_views(const uint8_t* video, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                               const int32_t* starts, int n, int f_skip, float* data, pc_stream s);
int64_t pc_detect_frames_views_ws_bytes(int n, int H, int W);
int     pc_detect_frames_views(const float* logits, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                               const int32_t* starts, int n, int f_skip, int row0, uint8_t* mask, int32_t* rec, void* ws, pc_stream s);
/* Per-frame instances (csrc/instances.hip; picons_amd/detect.py: DetectEngine(instances=K)): the masks pc_detect_frames* leave, split into
 * connected components on the device.  mask uint8 [F][H][W] (any non-zero byte is foreground; a frame may start at any byte address; frame
 * offsets are 64-bit), conn 4 or 8.  For each of the frames f0 .. f0 + nf - 1 the launch writes the WHOLE record of `inst` int32
 * [F][PC_INST_HDR + K * PC_INST_WORDS] and, if `imap` is not null, the WHOLE frame of imap uint8 [F][H][W]; no other frame is touched and
 * nothing has to be zeroed in front of it.  A null imap gives bit-identical records.
 *   header  [0] n_comp, the components of at least min_area pixels   [1] kept = min(n_comp, K)   [2] n_runs, the row runs (maximal horizontal
 *           foreground segments) of the frame   [3] flags, bit 0 = overflow
 *   slot r < K   area, x0, y0, x1, y1 (half-open box, full-frame coordinates), first = y * W + x of the component's first pixel in raster
 *           order; ranked by area descending, ties by first ascending; slots from kept on are all zeros
 *   imap    0 background, r + 1 on the component of rank r < kept, 255 on every other foreground pixel (below min_area or beyond K)
 * One 256-thread block per frame labels the runs in LDS, at most PC_INST_MAX_RUNS of them and PC_INST_MAX_ROWS rows.  A frame with more runs
 * (or whose labelling did not settle within its bound of n_runs + 1 iterations) is an OVERFLOW: flags = 1, n_comp = kept = 0, the slots zero,
 * n_runs the true count, imap 255 on all foreground; the caller falls back to the frame's single box.  Integer LDS atomics only, no
 * floating point: a record is bit-identical from run to run.  Refusals (PC_E_ARG before any HIP call, nothing allocated, enqueued on `s`
 * only): null mask or inst; F, H, W < 1; H > PC_INST_MAX_ROWS; W > 65535; H * W >= 2^31; f0 < 0, nf < 1, f0 + nf > F; conn not 4 or 8;
 * min_area < 1; K outside 1..32; inst not 4-byte aligned. */
#define PC_INST_HDR      4
#define PC_INST_WORDS    6
#define PC_INST_MAX_RUNS 2048
#define PC_INST_MAX_ROWS 2048
int     pc_frame_instances(const uint8_t* mask, int F, int H, int W, int f0, int nf, int conn, int min_area, int K, int32_t* inst,
                           uint8_t* imap, pc_stream s);
/* A confidence per instance (csrc/detect.hip, csrc/instances.hip; picons_amd/detect.py: DetectEngine(instance_scores=True)).
 * pc_frame_probs: the per-pixel probability in video order.  Geometry arguments, frame rules (f >= F neither read nor written, a frame the
 * launch does not address untouched, nothing to zero in front of it) and the merged logit m of a full-frame pixel are pc_detect_frames_views'
 * -- one device function (csrc/viewmerge.h) serves both kernels; the centre crop is the one view (h0, w0, 0) at stride n.  For every addressed
 * frame f < F the launch writes the WHOLE frame of `prob` uint16 [F][H][W]: q = __float2uint_rn(p * 65535.0f) with the fp32
 * p = 1 / (1 + expf(-m)), the expression the frame score sums; q = 0 for a pixel no view covers and for a NaN m.  So m = +-0.0 gives 32768,
 * +80 and +inf give PC_PROB_ONE, -80 and -inf give 0.  Grid and four-pixel groups of pc_detect_frames_views; no atomics, no LDS, no
 * workspace.  Refusals (PC_E_ARG before any HIP call): pc_detect_frames_views' list without row0 / rec / ws, a null prob, a prob that is not
 * 2-byte aligned.
 * pc_instance_scores: imap uint8 [F][H][W] as pc_frame_instances leaves it and prob as above (frames at any byte / element address) -> for
 * each of the frames f0 .. f0 + nf - 1, and no others, the WHOLE record of `out` int32 [F][PC_SCORE_WORDS * (K + 1)]: slot j = (lo, hi, npix),
 * the unsigned 64-bit sum of q over the slot's pixels and their number.  Slot r < K takes the pixels with map value r + 1, slot K every other
 * non-zero value (255, and any in K + 1 .. 254); the prob of a pixel with map value 0 is not read.  One 256-thread block per frame, integer
 * LDS atomics only: bit-identical from run to run, nothing to zero.  Refusals (PC_E_ARG before any HIP call): null imap / prob / out; F, H,
 * W < 1; H * W >= 2^31; f0 < 0, nf < 1, f0 + nf > F; K outside 1..32; prob not 2-byte or out not 4-byte aligned. */
#define PC_PROB_ONE    65535
#define PC_SCORE_WORDS 3
int     pc_frame_probs(const float* logits, int F, int H, int W, int S, const int32_t* views, int V, int view_stride, const int32_t* starts,
                       int n, int f_skip, uint16_t* prob, pc_stream s);
int     pc_instance_scores(const uint8_t* imap, const uint16_t* prob, int F, int H, int W, int f0, int nf, int K, int32_t* out, pc_stream s);
/* Mask overlaps between frames (csrc/instances.hip; picons_amd/detect.py: DetectEngine(instance_links=L), link_instance_tubes_by_mask).
 * pc_instance_overlaps: imap uint8 [F][H][W] as pc_frame_instances leaves it (a frame may start at any byte address; frame offsets are
 * 64-bit) -> for each of the frames f0 .. f0 + nf - 1, and no others, the WHOLE record of `out` int32 [F][L][K + 1][K + 1]: out[f][l][a][b]
 * is the number of pixels whose slot is a in frame f and b in frame f + l + 1.  The slots are pc_instance_scores': map value r + 1 <= K is
 * slot r, every other non-zero value (255, and any in K + 1 .. 254) slot K, value 0 belongs to nothing.  A lag with f + l + 1 >= F is written
 * as zeros; the partner frame may lie outside f0 .. f0 + nf - 1 as long as it is below F -- it is only read.  Nothing has to be zeroed in
 * front of the launch.  Grid (nf, L), one 256-thread block per (frame, lag); the partner's bytes of a four-pixel group are read only where
 * frame f holds foreground.  Integer LDS atomics only (per-wave bins of (K + 1)^2 int32, folded at the end), no global atomics, no floating
 * point: bit-identical from run to run.  Refusals (PC_E_ARG before any HIP call): null imap or out; F, H, W < 1; H * W >= 2^31; f0 < 0,
 * nf < 1, f0 + nf > F; K outside 1..32; L outside 1..PC_LINK_MAX_LAGS; out not 4-byte aligned. */
#define PC_LINK_MAX_LAGS 4
int     pc_instance_overlaps(const uint8_t* imap, int F, int H, int W, int f0, int nf, int K, int L, int32_t* out, pc_stream s);
/* Masks and maps of ranks as row runs (csrc/maskruns.hip; picons_amd/detect.py: DetectEngine.mask_runs, MaskRuns).  map uint8 [F][H][W] (a
 * frame may start at any byte address; frame offsets are 64-bit); only the frames f0 .. f0 + nf - 1, the RANGE, are read, and its rows are
 * numbered r = (f - f0) * H + y.  A RUN is a maximal horizontal segment of pixels with the same NON-ZERO byte value: value 0 belongs to no
 * run, two touching segments of different values are two runs.  For a 0 / 1 mask of pc_detect_frames* these are the foreground runs with
 * value 1, for the imap of pc_frame_instances the runs of each rank (r + 1) and of 255.
 * pc_mask_run_index writes the WHOLE of index int32 [nf * H + 1]: index[r] = the runs in the rows before row r of the range (raster order),
 * index[nf * H] = the range's total.  ws: pc_mask_run_ws_bytes(nf, H) bytes, 4-byte aligned, contents irrelevant before the call and
 * meaningless after it; nothing has to be zeroed.  Three launches: a count per row on a grid over bands of 32 rows (band sums into ws), one
 * block that scans the band sums, one launch that adds them back.
 * pc_mask_runs, with the index of the same map and range, writes runs uint32 [cap][PC_RUN_WORDS] in raster order: run index[r] + j is the
 * j-th run of row r from the left,
 *   runs[i][0] = r | value << 24        runs[i][1] = x0 | x1 << 16   (columns x0 .. x1 - 1: x1 half-open, at most 65535)
 * A run with i >= cap is not written and no byte at or behind runs[cap] is touched; cap = 0 with a non-null runs is legal and writes
 * nothing.  The true total is index[nf * H]: a buffer that is too small shows as total > cap, never as a corruption.  One launch on the
 * grid of the count.
 * No atomics of any kind, no floating point, nothing waits on another block, every loop's trip count fixed before it starts: bit-identical
 * from run to run.  pc_mask_run_ws_bytes is host arithmetic: -1 for nf < 1, H < 1 or nf * H > 2^24.  Refusals of the two calls (PC_E_ARG
 * before any HIP call, nothing allocated, enqueued on `s` only): null map / index / ws; null runs with cap > 0; cap < 0; F, H, W < 1;
 * W > 65535; f0 < 0, nf < 1, f0 + nf > F; nf * H > 2^24 (the row field); nf * H * W >= 2^31 (a run count is an int32: a longer video is
 * exported in ranges); index, runs or ws not 4-byte aligned. */
#define PC_RUN_WORDS 2
int64_t pc_mask_run_ws_bytes(int nf, int H);
int     pc_mask_run_index(const uint8_t* map, int F, int H, int W, int f0, int nf, int32_t* index, void* ws, pc_stream s);
int     pc_mask_runs(const uint8_t* map, int F, int H, int W, int f0, int nf, const int32_t* index, int64_t cap, uint32_t* runs, pc_stream s);
/* A map of a pass against a truth map (csrc/crosstab.hip; picons_amd/detect.py: DetectEngine.score).  pred and truth are two DIFFERENT
 * contiguous uint8 buffers [F][H][W] (a frame may start at any byte address on either side; frame offsets are 64-bit).  The SLOT of a pred
 * byte v is 0 for v = 0 (background), v for 1 <= v <= P, and P + 1 for anything above P ("other foreground": the 255 of a map of ranks, or
 * any value beyond); the slot of a truth byte is the same with A.  ANY non-zero truth byte is foreground -- deliberately unlike
 * pc_seg_frame_counts, whose intersection needs the truth value 1 (pred + gt == 2).
 * pc_map_crosstab writes, for each of the frames f0 .. f0 + nf - 1 and no others, EVERY cell of `out` int32 [F][P + 2][A + 2]:
 * out[f][p][a] = the pixels of frame f with pred slot p and truth slot a, cell [0][0] included, so the cells of a frame sum to H * W.
 * Nothing has to be zeroed in front of the call; the prior contents of out and ws are irrelevant.  ws: pc_map_crosstab_ws_bytes(nf, H, W,
 * P, A) bytes, 8-byte aligned, meaningless after the call.  Two launches: bpf blocks per frame (a function of H * W alone, at most 64)
 * leave one partial table each in ws, then one block per frame adds them in block order and writes [0][0] as H * W minus the rest.
 * Integer LDS atomics only (per-wave bins, folded at the end), no global atomics, no floating point, nothing waits on another block:
 * bit-identical from run to run.  pc_map_crosstab_ws_bytes is host arithmetic: -1 for nf, H or W < 1, H * W >= 2^31, P or A outside
 * 1..PC_CROSS_MAX_SLOTS.  Refusals of the call (PC_E_ARG before any HIP call): null pred, truth, out or ws; F, H, W < 1; H * W >= 2^31;
 * f0 < 0, nf < 1, f0 + nf > F; P or A outside 1..PC_CROSS_MAX_SLOTS; out not 4-byte aligned; ws not 8-byte aligned. */
#define PC_CROSS_MAX_SLOTS 32
int     pc_map_crosstab(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int f0, int nf, int P, int A, int32_t* out, void* ws,
                        pc_stream s);
int64_t pc_map_crosstab_ws_bytes(int nf, int H, int W, int P, int A);
/* The probability map of a pass against a truth map at every mask threshold at once (csrc/probhist.hip; picons_amd/detect.py:
 * DetectEngine.sweep).  prob uint16 [F][H][W] as pc_frame_probs, pc_detect_frames_scaled and pc_detect_frames_planes leave it (a frame may
 * start at any 2-byte address), truth uint8 [F][H][W] (any byte address; ANY non-zero byte is truth, as in pc_map_crosstab); frame offsets are
 * 64-bit.  thr: N HOST words, strictly ascending, each in 1..PC_PROB_ONE; they are read before the call returns and travel in the kernel
 * arguments, so the caller may free them at once.  With q a pixel's probability word and b the number of k with thr[k] <= q, the pixel is
 * positive at threshold k (q >= thr[k]) exactly if b > k.
 * pc_prob_truth_hist writes, for each of the frames f0 .. f0 + nf - 1 and no others, EVERY cell of `out` int32 [F][2][N + 1]: out[f][t][b] =
 * the pixels of frame f whose truth byte is zero (t = 0) or not (t = 1) and for which exactly b of the thresholds are <= q, cell [0][0]
 * included, so the cells of a frame sum to H * W.  Nothing has to be zeroed in front of the call; the prior contents of out and ws are
 * irrelevant.  ws: pc_prob_truth_hist_ws_bytes(nf, H, W, N) bytes, 8-byte aligned, meaningless after the call.  Two launches, as
 * pc_map_crosstab: bpf blocks per frame (a function of H * W alone, at most 64) leave one partial table each in ws, then one block per frame
 * adds them in block order and writes [0][0] as H * W minus the rest -- a pixel without truth below thr[0] costs no LDS traffic.  Integer LDS
 * atomics only (per-wave bins, folded at the end), no global atomics, no floating point, nothing waits on another block: bit-identical from
 * run to run.  pc_prob_truth_hist_ws_bytes is host arithmetic: -1 for nf, H or W < 1, H * W >= 2^31, N outside
 * 1..PC_SWEEP_MAX_THRESHOLDS.  Refusals of the call (PC_E_ARG before any HIP call): null prob, truth, thr, out or ws; F, H, W < 1;
 * H * W >= 2^31; f0 < 0, nf < 1, f0 + nf > F; N outside 1..PC_SWEEP_MAX_THRESHOLDS; a threshold word of 0; thresholds not strictly ascending;
 * prob not 2-byte, out not 4-byte, ws not 8-byte aligned. */
#define PC_SWEEP_MAX_THRESHOLDS 64
int64_t pc_prob_truth_hist_ws_bytes(int nf, int H, int W, int N);
int     pc_prob_truth_hist(const uint16_t* prob, const uint8_t* truth, int F, int H, int W, int f0, int nf, const uint16_t* thr, int N,
                           int32_t* out, void* ws, pc_stream s);
/* The kept probability map of a pass cut at a threshold word (csrc/probcut.hip; picons_amd/detect.py: DetectEngine.set_mask_threshold /
 * DetectEngine.recut).  prob uint16 [F][H][W] as pc_frame_probs, pc_detect_frames_scaled and pc_detect_frames_planes leave it (a frame may
 * start at any 2-byte address); frame offsets are 64-bit.  word in 1..PC_PROB_ONE; a pixel of probability word q is positive exactly if
 * q >= word -- pc_prob_truth_hist's rule, so a sweep and a cut cannot disagree on a pixel.
 * pc_prob_cut writes, for each of the frames f0 .. f0 + nf - 1 and no others, the whole frame of mask uint8 [F][H][W] (1 positive, 0 not; a
 * frame may start at any byte address; mask may be null, the records are then the same bits) and words 0..5 of the frame's record in rec
 * int32 [F][8]: [0] the count c of positive pixels, [1..4] their half-open box x0, y0, x1, y1 in frame coordinates (all zero for c == 0),
 * [5] the bits of the float32 score (float)((double)S / (65535.0 * (double)c)) with S the exact integer sum of q over the positive pixels
 * (S < 2^47: exact as an integer and as a double, so the score is a function of the input alone), 0.0f for c == 0.  WORDS 6 AND 7 ARE NOT
 * TOUCHED: they hold the frame's score row, written by the detect entry that ran first.  Nothing has to be zeroed in front of the call; the
 * prior contents of mask, rec and ws are irrelevant.  ws: pc_prob_cut_ws_bytes(nf, H, W) bytes, 8-byte aligned, meaningless after the
 * call.  Two launches, as pc_prob_truth_hist: bpf blocks per frame (a function of H * W alone, at most 64) write the mask and leave one
 * partial (count, box, sum) each in ws, then one thread per frame adds them in block order.  No global atomics, no LDS atomics, no floating
 * point that rounds except the final division, nothing waits on another block: bit-identical from run to run.  pc_prob_cut_ws_bytes is host
 * arithmetic: -1 for nf, H or W < 1, H * W >= 2^31.  Refusals of the call (PC_E_ARG before any HIP call): null prob, rec or ws; F, H,
 * W < 1; H * W >= 2^31; f0 < 0, nf < 1, f0 + nf > F; word outside 1..PC_PROB_ONE; prob not 2-byte, rec not 4-byte, ws not 8-byte aligned. */
int64_t pc_prob_cut_ws_bytes(int nf, int H, int W);
int     pc_prob_cut(const uint16_t* prob, int F, int H, int W, int f0, int nf, int word, uint8_t* mask, int32_t* rec, void* ws, pc_stream s);
/* A video's truth map painted from boxes on the device (csrc/truthboxes.hip; picons_amd/evalstep.py: BoxTruth; EvalEngine.add_video,
 * DetectEngine.score / sweep).  rects: DEVICE int32 [F][R][PC_BOX_WORDS], a row for every frame of the video, indexed by absolute frame; a
 * rect is (x0, x1, y0, y1, value) in frame coordinates, half-open.  truth uint8 [F][H][W], contiguous (a frame may start at any byte address,
 * H * W may be odd; frame offsets are 64-bit).
 * pc_paint_boxes writes, for each of the frames f0 .. f0 + nf - 1 and no other byte of truth, every byte of the frame exactly once: a pixel's
 * byte is the low byte of `value` of the LAST rect, in table order, that contains it, 0 if none does; with binary != 0 it is 1 instead of that
 * value.  That is what painting the rects in order gives (bbox[f, y0:y1, x0:x1] = value: a later annotation overwrites an earlier one).  A
 * rect paints nothing if x1 <= x0, y1 <= y0 or value & 255 == 0.  Nothing is read from truth: its prior contents are irrelevant and no fill
 * precedes the launch.
 * SAFE BY CONSTRUCTION: a rect word never becomes part of an address.  Each thread owns output bytes of a frame inside the checked range and
 * only tests whether a rect contains them, so a rect that reaches outside the frame -- or any 32-bit pattern at all -- is simply intersected
 * with the frame; the entry cannot write out of bounds whatever the table holds.
 * One launch (a map of more frames than the grid limit is cut into several): bpf blocks per frame (a function of H * W alone, at most 64),
 * the frame's R rects loaded once per block into LDS, each block strides over its share of the frame's four-pixel groups and stores them as
 * dwords where the address allows.  No atomics, no floating point, nothing waits on another block: bit-identical from run to run.  Refusals
 * (PC_E_ARG before any HIP call): null rects or truth; F, H, W < 1; H * W >= 2^31; R outside 1..PC_BOX_MAX; f0 < 0, nf < 1, f0 + nf > F; rects
 * not 4-byte aligned. */
#define PC_BOX_MAX   32     /* rects per frame */
#define PC_BOX_WORDS 5      /* x0, x1, y0, y1, value */
int     pc_paint_boxes(const int32_t* rects, int R, int F, int H, int W, int f0, int nf, int binary, uint8_t* truth, pc_stream s);
/* Detection on a resized working frame, results at native size (csrc/detectscale.hip; picons_amd/detect.py: DetectEngine.set_working_frame).
 * The views are crops of an Hs x Ws WORKING frame; mask, box, score and probability stand on the H x W NATIVE frame.
 * pc_resample_tables is HOST arithmetic with pc_resize_tables' call shape: it returns the word count 2 * (H + W) and writes `tab` if `cap`
 * words suffice; PC_E_ARG (-1) for a size < 1 or 2 * max(H, W) >= 2^24.  Layout: rows [H][2], then columns [W][2], each pair (i0, the bits
 * of the float32 w1).  For destination index d of D from a source of length L (rows: L = Hs, D = H; columns: L = Ws, D = W), half-pixel
 * centres (cv2.INTER_LINEAR / align_corners=False), exact in 64-bit integers: num = (2d + 1) * L - D, den = 2D, i0 = floor(num / den),
 * r = num - i0 * den; if i0 < 0: i0 = 0, r = 0; if i0 >= L - 1: i0 = L - 1, r = 0; w1 = (float)r / (float)den -- both exact in float32, the
 * division rounded once.  L == D gives i0 = d, w1 = 0: the identity.
 * pc_detect_frames_scaled: logits, views (crops of the Hs x Ws frame), view_stride, starts, n <= 32, f_skip, row0 are pc_detect_frames_views'
 * with (H, W) replaced by (Hs, Ws); dev_tab is the DEVICE copy of pc_resample_tables(Hs, Ws, H, W).
 *   1. Per working pixel the merged logit M and its cover count are pc_detect_frames_views' (csrc/viewmerge.h), bit for bit.
 *   2. Per native pixel (y, x) of the addressed frames, with (iy, wy1) = row pair y, (ix, wx1) = column pair x, wx0 = 1.0f - wx1,
 *      wy0 = 1.0f - wy1:   top = wx1 == 0 ? M[iy][ix] : M[iy][ix] * wx0 + M[iy][ix + 1] * wx1;   bot: the same on row iy + 1, formed only if
 *      wy1 != 0;   v = wy1 == 0 ? top : top * wy0 + bot * wy1.  Every product and sum is one fp32 round-to-nearest operation (no fma).  A tap
 *      of zero weight is not read: -0.0 and NaN pass through an identity resample, a NaN or an uncovered pixel under a zero weight poisons
 *      nothing.  The pixel is COVERED iff every tap that is read has cover count >= 1; an uncovered pixel is background, probability 0.
 *   3. From v on everything is pc_detect_frames_views': seg_positive, the whole frame of mask uint8 [F][H][W] (may be null), the half-open
 *      box in native coordinates, the score (fp32 sigmoid of v, summed in double: thread, wave, block partial in `ws`, a second launch adds the
 *      partials in block order), the 8-word record with rec[6] = row0 + c * V, the frame rules (f >= F neither read nor written, a frame not
 *      addressed untouched, nothing zeroed in front).  If `prob` is not null the same launch writes uint16 [F][H][W] with pc_frame_probs'
 *      conversion of v (NaN and uncovered: 0).
 * Three launches: the merge leaves M and the cover counts of the launch's n * 8 frames in `ws` (each logit fetched once), the resample walks
 * the native frame in groups of four pixels, the records kernel adds the partials.  No atomics of any kind: bit-identical from run to run,
 * with or without mask / prob.  ws: pc_detect_frames_scaled_ws_bytes(n, Hs, Ws, H, W) bytes, 8-byte aligned, contents irrelevant before and
 * meaningless after = pc_detect_frames_views_ws_bytes(n, H, W) + 16 + n * 8 * roundup4(Hs * Ws) * 5 (host-only; -1 for n outside 1..32, a
 * size < 1, Hs * Ws or H * W >= 2^31, 2 * max(H, W) >= 2^24).  Refusals (PC_E_ARG before any HIP call): pc_detect_frames_views' list on the
 * working frame, a null dev_tab, H or W < 1, H * W >= 2^31, 2 * max(H, W) >= 2^24, prob not 2-byte aligned. */
int64_t pc_resample_tables(int Hs, int Ws, int H, int W, int32_t* tab, int64_t cap);
int64_t pc_detect_frames_scaled_ws_bytes(int n, int Hs, int Ws, int H, int W);
int     pc_detect_frames_scaled(const float* logits, int F, int H, int W, int Hs, int Ws, int S, const int32_t* views, int V, int view_stride,
                                const int32_t* starts, int n, int f_skip, int row0, const int32_t* dev_tab, uint8_t* mask, uint16_t* prob,
                                int32_t* rec, void* ws, pc_stream s);
/* Overlapping clips in time, merged per frame (csrc/cliphop.hip, the rule in csrc/cliphop.h; picons_amd/detect.py: DetectEngine.set_clip_hop).
 * span = 8 * f_skip; hop is a multiple of f_skip in [f_skip, span] (f_skip <= 2^20).  Windows start at m * hop; window m is kept iff m == 0 or
 * (m - 1) * hop + span < F.  Clip starts are m * hop + j for every kept window and every phase j < f_skip with m * hop + j < F, in that
 * order; the clip with start s has index (s / hop) * f_skip + s % hop.  Frame f lies in the windows lo = max(0, ceil((f - span + 1) / hop))
 * .. hi = min(f / hop, windows - 1): at least 1, at most M = ceil(span / hop) <= 8, with pairwise distinct m % M.  hop == span is the cut of
 * pc_detect_frames*: every frame in one window.
 * pc_clip_hop_starts is HOST arithmetic: it returns the clip count and writes `starts` if it is not null and `cap` entries suffice;
 * PC_E_ARG (-1) for F < 1 or a bad f_skip / hop.
 * pc_clip_planes: logits, views (crops of the Hs x Ws frame: the working frame, or the native one), view_stride, starts, n <= 32 are
 * pc_detect_frames_views'.  Frame k of clip c goes to slot (starts[c] / hop) % M of frame starts[c] + k * f_skip in plane float32
 * [M][F][pstride], pstride = Hs * Ws rounded up to 4: the merged logit of pc_detect_frames_views (csrc/viewmerge.h) bit for bit, 0.0f where no
 * view covers, in 16-byte stores, each logit fetched once.  cover uint8 [pstride], the views that cover each pixel -- the same for every
 * clip of a video --, is written if it is not null.  A frame >= F is neither read nor written; a (slot, frame) the launch does not address
 * is not touched; two clips of one launch never address the same one, so there are no atomics, nothing is zeroed and the order of a
 * video's launches does not matter.  pc_clip_planes_bytes (host-only; -1 for a size < 1, Hs * Ws >= 2^31, a bad f_skip / hop) =
 * M * F * pstride * 4 + pstride: the planes, then the cover.  Refusals (PC_E_ARG before any HIP call): null logits, views, starts or plane;
 * pc_detect_frames_views' checks of F, Hs, Ws, S, V, n, view_stride, f_skip, views and negative starts; a bad hop; a start below F that is
 * no clip start of the rule; logits or plane not 16-byte, cover not 4-byte aligned; a cover together with starts[0] >= F.
 * pc_detect_frames_planes: for each of the frames f0 .. f0 + nf - 1 (nf <= PC_PLANES_MAX_FRAMES) and no others, steps 2 and 3 of
 * pc_detect_frames_scaled with M[y][x] the mean of the frame's plane value over the windows lo .. hi in ascending order -- the first value as
 * it is, the others added in fp32 round-to-nearest, one fp32 division by the count when it is above 1 -- and the cover byte that of the
 * video.  A slot no window filled is never read.  dev_tab: the device copy of pc_resample_tables(Hs, Ws, H, W), the identity for equal
 * sizes, where every output is the unscaled path's bit for bit.  rec[6] = row0 + V * (lo * f_skip + f % f_skip), the score row of the first
 * clip that holds the frame; rec[7] = 0.  mask and prob may be null; the records are the same either way.  Two launches, no atomics.
 * ws: pc_detect_frames_planes_ws_bytes(nf, H, W) bytes (host-only; -1 for nf outside 1..PC_PLANES_MAX_FRAMES, a size < 1, H * W >= 2^31),
 * 8-byte aligned, contents irrelevant before and meaningless after.  Refusals (PC_E_ARG before any HIP call): null plane, cover, dev_tab, rec
 * or ws; F < 1; a size < 1; Hs * Ws or H * W >= 2^31; 2 * max(H, W) >= 2^24; V outside 1..32; a bad hop; f0 < 0, nf outside
 * 1..PC_PLANES_MAX_FRAMES, f0 + nf > F; row0 < 0 or row0 + V * clips > INT_MAX; plane not 16-byte, cover, dev_tab or rec not 4-byte, ws not
 * 8-byte, prob not 2-byte aligned. */
#define PC_PLANES_MAX_FRAMES 256
int64_t pc_clip_hop_starts(int F, int f_skip, int hop, int32_t* starts, int64_t cap);
int64_t pc_clip_planes_bytes(int F, int Hs, int Ws, int f_skip, int hop);
int     pc_clip_planes(const float* logits, int F, int Hs, int Ws, int S, const int32_t* views, int V, int view_stride, const int32_t* starts, int n,
                       int f_skip, int hop, float* plane, uint8_t* cover, pc_stream s);
int64_t pc_detect_frames_planes_ws_bytes(int nf, int H, int W);
int     pc_detect_frames_planes(const float* plane, const uint8_t* cover, int F, int H, int W, int Hs, int Ws, int V, int f_skip, int hop, int f0,
                                int nf, int row0, const int32_t* dev_tab, uint8_t* mask, uint16_t* prob, int32_t* rec, void* ws, pc_stream s);
/* cv2.resize on uint8 images [n][H][W][C] -> [n][Ho][Wo][C] (C <= 4), the calls of the reference's loaders:
 * datasets/jhmdb_dataloader.py:252 (frames, INTER_AREA 320x240 -> 256x256), :267,:281 (puppet masks, INTER_NEAREST),
 * :192,:208 and ucf_dataloader.py:165,171 (224 crop -> frame size, INTER_LINEAR; the identity at 224).  OpenCV's 8-bit
 * algorithm restated (csrc/inputpipe.hip has the rules).  pc_resize_tables is HOST arithmetic (no GPU needed): it writes the
 * int32 coordinate / coefficient table for one (interpolation = cv2 flag 0 nearest | 1 linear | 3 area, sizes) into `tab` if
 * `cap` words suffice and returns the word count; the caller uploads it once and passes the device copy to pc_resize_u8.
 * binarize != 0: the result is (value > 0) of resizing a non-negative mask in float, i.e. 1 where a tap with a positive
 * weight meets a positive sample (`cv2.resize(bbox_img, ...) > 0`, ucf_dataloader.py:170-172). */
int64_t pc_resize_tables(int interpolation, int H, int W, int Ho, int Wo, int32_t* tab, int64_t cap);
int pc_resize_u8(const uint8_t* src, int n, int H, int W, int C, int Ho, int Wo, const int32_t* dev_tab, int binarize,
                 uint8_t* dst, pc_stream s);
int pc_fill(float* p, int64_t n, float v, pc_stream s);
int pc_axpy(float* y, const float* x, int64_t n, float a, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Capsule head (capsules_ucf101.py:290-331, 108-211): votes + 3-iteration EM routing, one
 * wave per spatial position, votes recomputed from poses and W held in LDS.
 *  x      [npos][B*17]   primary caps output (poses B*16 then activations B)
 *  W      [B][C][4][4], beta_u [C][16], beta_a [C]
 *  out    [npos][C*17]   (mu C*16 then a_out C)
 * backward: hand-derived reverse of all iterations (autograd equivalent), per-block partial
 * parameter grads in ws then reduced; dW/dbeta_u/dbeta_a accumulated (+=).
 *  state  optional, pc_em_state_floats(npos) floats, 16-byte aligned: the forward leaves every iteration's routing state
 *         there (assignments, means, variances, ...: 21 KB per position) and a backward given the same buffer loads it
 *         instead of running the routing iterations again; NULL = no state kept / the backward recomputes the forward. */
int64_t pc_em_ws_floats(int npos, int B, int C);
int64_t pc_em_state_floats(int npos);
int pc_em_routing_fwd(const float* x, const float* W, const float* beta_u, const float* beta_a,
                      int npos, int B, int C, float* out, float* state, pc_stream s);
int pc_em_routing_bwd(const float* x, const float* W, const float* beta_u, const float* beta_a,
                      const float* dout, int npos, int B, int C, float* dx, float* dW,
                      float* dbeta_u, float* dbeta_a, float* ws, const float* state, pc_stream s);

/* class-capsule masking (capsules_ucf101.py:438-484):
 *  actor_prediction[b][c] = mean_pos act; mask row: labeled -> one-hot(cls), unlabeled ->
 *  ones (mode 0) or one-hot(argmax pred) (mode 1); eval (mode 2): argmax for all rows.
 *  masked[b,pos,c*16+h] = pose * mask[b][c];  mask is written out for the backward. */
int pc_class_mask_fwd(const float* caps, int Bn, int npos_per_b, int C, const float* cls,
                      const int32_t* labeled, int mode, float* actor_pred, float* mask,
                      float* masked, pc_stream s);
/* dcaps = [dmasked*mask , dactor_pred/npos_per_b] */
int pc_class_mask_bwd(const float* dmasked, const float* dactor_pred, const float* mask, int Bn,
                      int npos_per_b, int C, float* dcaps, pc_stream s);

/* `smooth` ConvTranspose3d(128->1,k3,p1) second stage (capsules_ucf101.py:373,509): the 27 tap
 * projections proj[n,t,h,w,32] (from pc_conv_fwd with Co=27) are summed at their offsets:
 *  out[n,t,h,w] = bias + sum_tap proj[n, (t,h,w)+pad-k(tap), tap]   and the adjoint. */
int pc_tapsum_fwd(const float* proj, int N, int T, int H, int W, const float* bias, float* out, pc_stream s);
int pc_tapsum_bwd(const float* dout, int N, int T, int H, int W, float* dproj, pc_stream s);

/* Collapsed decoder tail: upsample4 -> Dropout3d -> smooth (capsules_ucf101.py:504-509) are three linear ops, so
 * they run as ONE 128->27 transposed conv with per-sample combined weights
 *   Wc[n][ci][tap][j] = sum_co W4[ci][co][tap] * cs[n][co] * Wp[co][j],  bc[n][j] = sum_co b4[co]*cs[n][co]*Wp[co][j]
 * followed by pc_tapsum_fwd.  W4 = upsample4.weight (Ci,Co,taps), Wp = smooth.weight (Co,J=27), cs = Dropout3d scale
 * (N,Co) or NULL.  Wt [N][Ci][taps][32] is the dgrad layout, Wf [N][32][taps][Ci] the forward layout, bc [N][32]. */
int pc_tail_combine(const float* W4, const float* b4, const float* cs, const float* Wp, int N, int Ci,
                    int Co, int taps, int J, float* Wt, float* Wf, float* bc, pc_stream s);
/* sums[n][32] = per-sample column sums of dproj [N][rows_per_n][32] */
int pc_tail_colsum(const float* dproj, int N, int64_t rows_per_n, float* sums, pc_stream s);
/* G [N][Ci][taps][32] = per-sample dWc (from pc_conv_wgrad) -> upsample4.weight/bias and smooth.weight/bias grads (+)= */
int pc_tail_grads(const float* G, const float* sums, const float* W4, const float* b4, const float* cs,
                  const float* Wp, int N, int Ci, int Co, int taps, int J, int center, float* dW4,
                  float* db4, float* dWp, float* dbp, int accum, pc_stream s);
/* the same with the smooth-weight gradient's N * Ci/8 block partials stored in ws (pc_tail_grads_ws_floats floats, no initialisation needed) and
 * added in block order instead of fp32 atomics: bit-identical from run to run (round 6).  ws == NULL: pc_tail_grads. */
int64_t pc_tail_grads_ws_floats(int N, int Ci, int Co);
int pc_tail_grads_ws(const float* G, const float* sums, const float* W4, const float* b4, const float* cs,
                     const float* Wp, int N, int Ci, int Co, int taps, int J, int center, float* dW4,
                     float* db4, float* dWp, float* dbp, int accum, float* ws, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Fused loss: everything main_ucf101.py:89-148 computes from (output, flip_op, loc_msk):
 * BCEWithLogits + Dice on labeled rows, equal-weight L2, bv (utils/helpers.py:8-67) and gv
 * (:70-95) attentive masks with their weighted MSE, combined as the reference does, plus
 * d(total)/d(output), d(total)/d(flip_op).  Masks are detached, like the reference's numpy. */
typedef struct pc_loss_desc {
    int32_t B, T, H, W;             /* T must be 8 (utils/helpers.py:14) */
    int32_t bv, gv, n_frames, predict_maps, jhmdb;
    float   lower_thresh, upper_thresh;   /* <0 = None */
    float   bv_wt, gv_wt, wt_loc, wt_cons, wt_ramp;
} pc_loss_desc;
int64_t pc_loss_ws_floats(const pc_loss_desc* d);
/* output, flip_op: [B][T][H][W] logits (flip_op still W-mirrored, as the model returns it);
 * seg [B][T][H][W]; labeled[B] 0/1.  scalars[8] = {loc, cons, bce, dice, l2, lv1+lv2, lg, n_labeled};
 * total adds wt_cls*spread on the host side.  mask_bv/mask_gv optional outputs (may be NULL). */
int pc_consistency_loss(const pc_loss_desc* d, const float* output, const float* flip_op,
                        const float* seg, const int32_t* labeled, float* scalars, float* d_output,
                        float* d_flip_op, float* mask_bv, float* mask_gv, float* ws, pc_stream s);
/* standalone masks behind utils.helpers.measure_pixelwise_var_v2 / measure_pixelwise_gradient */
int pc_var_mask(const float* pred, const float* flip_pred, int B, int T, int H, int W, int n_frames,
                int use_sig, float* mask, float* ws, pc_stream s);
int pc_grad_mask(const float* pred, int B, int T, int H, int W, float lower, float upper,
                 float* mask, float* ws, pc_stream s);
/* SpreadLoss (utils/losses.py:14-37) on labeled rows: out[2] = {loss, absloss}; dx (+)= wt*dloss/dx */
int pc_spread_loss(const float* x, const float* cls, const int32_t* labeled, int Bn, int C, float m,
                   float wt, float* out, float* dx, pc_stream s);

/* fused Adam over a flat buffer (optim.Adam(lr, weight_decay=0, eps=1e-6), main_ucf101.py:416);
 * gscale folds the 1/world_size of the DP mean. */
int pc_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1,
                 float b2, float eps, int step, float gscale, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Row-spectral PrimaryCaps (capsules_ucf101.py:43-49: Conv2d 832 -> 512+32, 9x9, stride 1).  A real DFT
 * of length P = image width along the rows turns the kx taps into a product per frequency; what is left
 * is a 9x1 conv with complex channels per frequency u = 0..P/2.  The complex product is taken in its
 * three-multiplication form (X = Xr + i Xi, conj(W) = Wr - i Wi):
 *     t0 = (Xr + Xi) Wr,  t1 = Xi (Wr - Wi),  t2 = Xr (Wr + Wi);   Re = t0 - t1,  Im = t0 - t2,
 * so the whole layer is ONE grouped real conv for pc_conv_fwd / pc_conv_wgrad (3 groups per complex frequency,
 * 1 for DC / Nyquist; Ci -> Co, 9x1 taps): a quarter of the direct form's multiply-adds, equal to it in exact arithmetic.
 * The sums/differences of the operands and results are folded into the DFT matrices.  These three
 * HBM-bound helpers are the rest of it. */
/* out[r][o][c] = sum_i M[o][i] * in[r][i][c] (+ bias[c]; activation on channels >= act_c0; accum adds
 * the old value first): a small dense matrix along one tensor axis.  Element offsets (floats):
 * in:  r*in_sr  + (i / in_split)*in_hi   + (i % in_split)*in_lo  + c
 * out: r*out_sr + (o / out_split)*out_hi + (o % out_split)*out_lo + c */
typedef struct pc_axis_desc {
    int32_t R, I, O, C;
    int32_t in_split, out_split, act, act_c0, accum;
    int32_t in_sr, in_hi, in_lo, out_sr, out_hi, out_lo;
} pc_axis_desc;
int pc_axis_linear(const pc_axis_desc* d, const float* in, const float* M, const float* bias, float* out, pc_stream s);
/* weights in a kernel layout in[A][KY*KX][B] -> weight planes [A][KY][B]: three per complex frequency,
 *   V0 = Wr, V1 = Wr - Wi, V2 = Wr + Wi,  Wr = sum_kx in*tw[u][kx][0], Wi = sum_kx in*tw[u][kx][1]
 * (tw = cos, -sin of 2*pi*u*kx/P), followed by ONE plane (Wr) for each of the Ur trailing frequencies of tw whose spectrum
 * is real (DC and, for even P, Nyquist: X and W have no imaginary part there, so one real product is the whole term).
 * in = [Co][taps][Ci] gives the forward GEMM weights, in = [Ci][taps][Co] the dgrad GEMM weights. */
int pc_wspec_fwd(const float* in, const float* tw, int A, int B, int KY, int KX, int U, int Ur, float* out, pc_stream s);
/* adjoint: kg[a][ky*KX+kx][b] = sum_u tw[u][kx][0]*(d0+d1+d2) + tw[u][kx][1]*(d2-d1) over the complex frequencies plus
 * tw[u][kx][0]*d0 over the real ones; dV in the plane order of pc_wspec_fwd */
int pc_wspec_bwd(const float* dV, const float* tw, int A, int B, int KY, int KX, int U, int Ur, float* kg, pc_stream s);

/* The same two maps straight from / to the reference's master layout w[A][B][KY][KX] (OIHW, taps contiguous), so the
 * 36.7 M-element PrimaryCaps weight needs no kernel-layout copies: rows [a0, a0 + Acnt) of an Atot-row weight (pose and
 * activation capsules are two tensors).  out_f = planes [g][Atot][KY][B] (forward GEMM), out_t = [g][B][KY][Atot] (dgrad
 * GEMM); either may be NULL.  The adjoint reads plane gradients in the out_f layout and writes (accum: adds to) dw. */
int pc_wspec_master_fwd(const float* w, const float* tw, int Acnt, int a0, int Atot, int B, int KY, int KX, int U, int Ur,
                        float* out_f, float* out_t, pc_stream s);
/* pc_wspec_master_fwd with the planes written as the three bf16 terms of every value (pc_split_planes' format, term p at + p * plane_stride
 * elements) for pc_conv_fwd_x6: no fp32 copy of the 2 x 167 M-element PrimaryCaps weight planes exists in that mode */
int pc_wspec_master_planes(const float* w, const float* tw, int Acnt, int a0, int Atot, int B, int KY, int KX, int U, int Ur,
                           uint16_t* out_f, uint16_t* out_t, int64_t plane_stride, pc_stream s);
int pc_wspec_master_bwd(const float* dV, const float* tw, int Acnt, int a0, int Atot, int B, int KY, int KX, int U, int Ur,
                        float* dw, int accum, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Merged decoder tail (capsules_ucf101.py:504-509).  upsample4 -> Dropout3d -> smooth composes, per dimension, into one
 * stride-2 transposed conv with five taps k5 = k4 + ks (o = 2i - 2 + k5) and ONE output channel; the single term that
 * would pass through the cropped position m = -1 of upsample4's output (input index 0, k4 = 0, only in tap k5 = 2) is
 * left out of that tap's weight for the positions whose index is 0 in that dimension.  The positions therefore fall into
 * 8 classes z = 4*(it==0) + 2*(ih==0) + (iw==0), each with its own 128 x 125 weight matrix, and
 * cols[n][i][slot] = x[n][i][:] . W5[n][z(i)][:][slot], slot = (k5t*5 + k5h)*5 + k5w (125, padded to 128), is one grouped
 * 1x1 GEMM per class over its sub-lattice for pc_conv_fwd; these helpers are the rest. */
/* wf [N][32][27][Ci] (pc_tail_combine's forward layout) -> W5f [N][8][128][Ci] (forward GEMM), W5t [N][8][Ci][128] (dgrad GEMM) */
int pc_tail6_weights(const float* wf, int N, int Ci, float* W5f, float* W5t, pc_stream s);
/* out[n][o] = bsm[0] + sum_{ks: o+1-ks in grid} bc[n][ks] + sum of the <= 27 entries of cols [N][It][Ih][Iw][128] that
 * land on o = 2i - 2 + k5; out is [N][2It][2Ih][2Iw] */
int pc_tail6_gather(const float* cols, const float* bc, const float* bsm, int N, int It, int Ih, int Iw, float* out, pc_stream s);
/* the transpose: dcols[n][i][slot] = dout[n][2i - 2 + k5] (0 where that output does not exist) */
int pc_tail6_scatter(const float* dout, int N, int It, int Ih, int Iw, float* dcols, pc_stream s);
/* dW5 [N][8][Ci][128] -> gradient of the combined weights Gc [N][Ci][27][32] in the layout pc_tail_grads consumes */
int pc_tail6_wgrad_map(const float* dW5, int N, int Ci, float* Gc, pc_stream s);
/* the same from the classes' K-slice workspaces (pc_wgrad_desc.ws_slices, one launch per class with the N clip-passes as batched problems,
 * gbstride = Ci*128): ws = [z][k < nslices8[z]][N][Ci][128] back to back, nslices8[z] = 0 for an empty class.  A class's images are added in slice
 * order INTO ITS IMAGE 0 (ws is modified; the next pc_conv_wgrad into it rewrites image 0), the class sums in class order -- no fp32 atomics */
int pc_tail6_wgrad_map_slices(float* ws, const int32_t* nslices8, int N, int Ci, float* Gc, pc_stream s);
/* sums[n][ks] = sum of dout[n][o] over the outputs whose smooth tap ks reads an in-grid position (what pc_tail_colsum
 * gives on the 27-channel form) */
int pc_tail6_bias_sums(const float* dout, int N, int It, int Ih, int Iw, float* sums, pc_stream s);
/* the same without atomics: ws (pc_tail6_bias_sums_ws_floats floats, no initialisation needed) takes one partial row per block, a second
 * kernel adds them in block order.  ws == NULL: pc_tail6_bias_sums. */
int64_t pc_tail6_bias_sums_ws_floats(int N, int It, int Ih, int Iw);
int pc_tail6_bias_sums_ws(const float* dout, int N, int It, int Ih, int Iw, float* sums, float* ws, pc_stream s);

/* ------------------------------------------------------------------------------------------
 * Op-list runner: the host builds the step as a flat list of POD ops once (shape inference and
 * arena planning in Python) and the library replays it with no per-op host round trip. */
typedef struct pc_op {
    int32_t  kind;                  /* PC_OP_* */
    int32_t  i[48];
    float    f[8];
    int32_t  lane;                  /* which of the runner's streams the op is enqueued on (0 = main) */
    uint64_t p[12];                 /* device pointers */
    int64_t  l[4];
} pc_op;
enum {
    PC_OP_CONV = 1, PC_OP_WGRAD, PC_OP_BN_FINALIZE, PC_OP_BN_APPLY, PC_OP_BN_EVAL_STAT, PC_OP_BN_BWD,
    PC_OP_POOL_FWD, PC_OP_POOL_BWD, PC_OP_CHSCALE, PC_OP_ACT_BWD, PC_OP_TO_NDHWC, PC_OP_TO_NCDHW,
    PC_OP_TRANSPOSE, PC_OP_FILL, PC_OP_AXPY, PC_OP_EM_FWD, PC_OP_EM_BWD, PC_OP_CMASK_FWD,
    PC_OP_CMASK_BWD, PC_OP_TAPSUM_FWD, PC_OP_TAPSUM_BWD, PC_OP_LOSS, PC_OP_SPREAD, PC_OP_ADAM,
    PC_OP_TAIL_COMBINE, PC_OP_TAIL_COLSUM, PC_OP_TAIL_GRADS, PC_OP_COL2IM,
    PC_OP_AXIS,                     /* i[0..14] = pc_axis_desc; p = in, M, bias, out */
    PC_OP_WSPEC_FWD,                /* i = A, B, KY, KX, U, Ur; p = in, tw, out */
    PC_OP_WSPEC_BWD,                /* i = A, B, KY, KX, U, Ur; p = dV, tw, kg */
    PC_OP_WSPEC_MASTER_FWD,         /* i = Acnt, a0, Atot, B, KY, KX, U, Ur; p = w, tw, out_f, out_t */
    PC_OP_WSPEC_MASTER_BWD,         /* i = Acnt, a0, Atot, B, KY, KX, U, Ur, accum; p = dV, tw, dw */
    PC_OP_TAIL6_WEIGHTS,            /* i = N, Ci; p = wf, W5f, W5t */
    PC_OP_TAIL6_GATHER,             /* i = N, It, Ih, Iw; p = cols, bc, bsm, out */
    PC_OP_TAIL6_SCATTER,            /* i = N, It, Ih, Iw; p = dout, dcols */
    PC_OP_TAIL6_WGRAD_MAP,          /* i = N, Ci, sliced, nslices[8]; p = dW5 (sliced: the classes' K-slice workspaces), Gc */
    PC_OP_TAIL6_BIAS_SUMS,          /* i = N, It, Ih, Iw; p = dout, sums, ws (or 0) */
    PC_OP_TRANSPOSE_MULTI,          /* p[0] = HOST pointer to pc_transpose_job[i[0]] (kept alive by the owner of the list) */
    PC_OP_FORK,                     /* i[0] = lane bitmask: those lanes wait for everything enqueued so far on lane i[1] (0 by default) */
    PC_OP_JOIN,                     /* i[0] = lane bitmask: lane 0 waits for everything enqueued on those lanes */
    PC_OP_WGRAD_MULTI,              /* p[0] = HOST pointer to pc_wgrad_job[i[0]] (kept alive by the owner of the list): pc_conv_wgrad_multi */
    PC_OP_WINO_CONV,                /* i[0..15] = pc_wino_desc; p = in, U, bias, out, bnpart */
    PC_OP_WINO_WEIGHTS,             /* i = O, I, KT, flip, m (4: pc_wino4_weights); l = sO, sT, sI; p = w, U */
    PC_OP_CONV_X6,                  /* i = pc_conv_desc (flags with PC_F_X6); l[0] = plane stride, l[1] = workspace floats; p = in, wplanes, bias, cscale, out, bnpart, ws (0: none) */
    PC_OP_SPLIT_PLANES,             /* l = n, plane stride; p = src, planes */
    PC_OP_SPLIT_PLANES_MULTI,       /* p[0] = HOST pointer to pc_split_job[i[0]] (kept alive by the owner of the list) */
    PC_OP_WSPEC_MASTER_PLANES,      /* i = Acnt, a0, Atot, B, KY, KX, U, Ur; l[0] = plane stride; p = w, tw, out_f planes, out_t planes */
    PC_OP_BN_FIN_APPLY,             /* i = npg, groups, C, ldz, ldy, relu; l = count per group, rows; f = eps, momentum; p = part, gamma, beta, running_mean, running_var, stat, z, y */
    PC_OP_WGRAD_FOLD,               /* i[0] = nslices; l[0] = image floats; p = ws: pc_wgrad_fold */
    PC_OP_WINO_WEIGHTS_MULTI,       /* p[0] = HOST pointer to pc_wino_weights_job[i[0]] (kept alive by the owner of the list) */
    PC_OP_VAL_METRICS,              /* i = B, C; l[0] = pix; p = output, loc_msk, predicted_action, action, record, ws: pc_val_metrics */
    PC_OP__COUNT
};
#define PC_MAX_LANES 8
/* Replays the list on one stream (lane tags ignored: FORK/JOIN are no-ops, order = list order). */
int pc_run_ops(const pc_op* ops, int n, pc_stream s);
/* Replays the list over `nlanes` HIP streams: op k is enqueued on lanes[ops[k].lane]; the independent
 * branches of an Inception module (pytorch_i3d.py:149-154) and their backward run concurrently between
 * a FORK and the matching JOIN.  Lanes >= nlanes fold onto lane 0.  Every list must end joined. */
int pc_run_ops_lanes(const pc_op* ops, int n, const pc_stream* lanes, int nlanes);
/* `target` waits for everything enqueued so far on each of the nlanes streams (one persistent event per lane, no host sync):
 * how a gradient bucket's all-reduce stream is put behind every lane of a step replayed in segments (dist.GradReducer.launch;
 * the reference has no counterpart -- it is single-GPU, main_ucf101.py:171-184). */
int pc_streams_fanin(pc_stream target, const pc_stream* lanes, int nlanes);
/* Destroys the events the calling thread's replays created (FORK / JOIN, fan-in, the timing pool; VERDICT r1 weak 12: they are
 * thread-local and otherwise live until the process ends).  Callable at any time the streams are idle; later calls re-create them. */
int pc_release_thread_events(void);
/* same, with a hipEvent pair around every op of `kind` on the stream that op runs on (for PC_OP_CONV, whose ops are
 * one kernel each, the pair rides in the kernel's own dispatch and brackets exactly the kernel; other kinds are
 * bracketed by recorded events); returns elapsed ms summed over those ops in *ms and their count in *count (bench.py
 * roofline leg).  Synchronises all lanes before returning (unless ms == NULL, see below). */
int pc_run_ops_timed(const pc_op* ops, int n, int kind, float* ms, int* count, const pc_stream* lanes, int nlanes);
/* With ms == NULL pc_run_ops_timed does not synchronise: the event pairs stay pending (per host thread) until this call
 * waits for them and returns their summed elapsed ms and their number. */
int pc_run_ops_timed_collect(float* ms, int* count);

#ifdef __cplusplus
}
#endif
#endif
