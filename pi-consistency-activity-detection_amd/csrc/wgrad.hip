// Weight gradients of the gather-GEMM convolution family for gfx950 (the forward / dgrad kernels are in conv.hip): the generic split-K
// kernel, the row-segment kernels (KW = 3 / 9), the 4-channel stem kernels, their fp32-on-bf16-matrix-core forms, and ONE host dispatch
// (pc_conv_wgrad, pc_conv_wgrad_multi) that the reporter (pc_wgrad_variant) and the accounting (pc_wgrad_work) read as well.
#include "conv_common.h"
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <algorithm>
#include <vector>

// Weight gradient: G[m][n] += sum_pos D[pos][m] * S[gather(pos, tap(n))][cs(n)], n = tap*Cs + cs.
// K (positions) is split into slices; fp32 atomics, or K-slice images in a workspace added in slice order, combine them.
namespace {

struct WgK {
    const float* D; const float* S; float* g;
    int N, Tq, Hq, Wq, Cd, ldd, Ts, Hs, Ws, Cs, lds;
    int istr[3], ntap[3], ioff0[3], istep[3], wk0[3];
    int KH, KW, NtotFull;
    int P, Ntot, chunks_per_split, nchunks;
    int mbase, mend;                 // rows [mbase, mend) of D's channels handled by this launch
    int store;                       // one K slice: plain stores instead of atomics
    int nsplit, dbs, sbs, gbs;       // blockIdx.z = problem * nsplit + K slice; pointers advance by these strides per problem
    int dlat, Td, Hd, Wd, doff[3];   // dlat: D is a sub-lattice (Tq,Hq,Wq) at doff of a [N][Td][Hd][Wd] tensor instead of dense
    int mt, ntl;                     // tiles along Cd and along the columns; the grid is 1-D: mt * ntl * problems * slices blocks
    long long wss;                   // > 0: g is a workspace of K-slice images wss floats apart -- slice k leaves its partial sums in image k with
                                     // plain stores and the gradient re-layout adds the images in slice order (no atomics: bit-identical reruns)
};

// X6: the multiplications on the bf16 matrix cores (conv_x6.hip's scheme; both operands are activations, so both are split in registers: a
// lane's MFMA operand is eight consecutive positions of one column of the [position][column] tiles, read with eight ds_read_b32)
template <int BM, int BN, int ABL, int KB, bool X6 = false, bool HILO = true>
__device__ __forceinline__ void wgrad_body(const WgK& p, const int lid) {
    constexpr int BK = KB;                           // positions per chunk (shadows the file-level BK)
    constexpr int TM = BM / 64, TN = BN / 64;        // 2x2 waves
    static_assert(TM >= 1 && TN >= 1, "tile");
    __shared__ __attribute__((aligned(16))) float Ds[2][BK][BM];
    __shared__ __attribute__((aligned(16))) float Ss[2][BK][BN];
    __shared__ int4 ptab[3][BK];                     // per chunk: n, t0, h0, w0 of its 32 positions
    __shared__ int drow[3][BK];                      // row of D for each position (sub-lattice launches)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    // lid: logical block id of this problem (XCD-aware order: the blocks of one K slice -- every tile reads the same rows of D, and
    // overlapping rows of S -- get consecutive ids, i.e. run on one XCD and share its L2)
    const int tiles = p.mt * p.ntl, tile = lid % tiles, bz = lid / tiles;
    const int m0 = p.mbase + (tile % p.mt) * BM, n0 = (tile / p.mt) * BN;
    // bz = problem * nsplit + K slice
    const int prob = bz / p.nsplit, slice = bz - prob * p.nsplit;
    const int c_begin = slice * p.chunks_per_split;
    const int c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    if (c_begin >= c_end) return;
    const float* Dp = p.D + (size_t)prob * p.dbs;
    const float* Sp = p.S + (size_t)prob * p.sbs;
    float* gp = p.g + (size_t)prob * p.gbs + (size_t)slice * p.wss;

    // column decode for the S tile (constant over the K loop)
    constexpr int SC4 = BN / 4, DC4 = BM / 4;          // float4 columns per row
    constexpr int SRP = 256 / SC4, DRP = 256 / DC4;    // rows covered per pass
    const int scol = (tid % SC4) * 4, srow0 = tid / SC4;
    const int dcol = (tid % DC4) * 4, drow0 = tid / DC4;
    const int ncol = n0 + scol;
    const bool nval = ncol < p.Ntot;
    const int tap = nval ? ncol / p.Cs : 0, cs = ncol - tap * p.Cs;
    const int tapHW = p.ntap[1] * p.ntap[2];
    const int a_ = tap / tapHW, rem = tap - a_ * tapHW, b_ = rem / p.ntap[2], c_ = rem - b_ * p.ntap[2];
    const int dt = a_ * p.istep[0], dh = b_ * p.istep[1], dw = c_ * p.istep[2];
    const bool mval = (m0 + dcol) < p.mend;
    (void)rem;

    auto ptab_fill = [&](int c) {
        if (tid < BK) {
            const int pos = c * BK + tid;
            int4 info = make_int4(-1, 0, 0, 0);
            if (c < c_end && pos < p.P) {
                int m = pos;
                const int wq = m % p.Wq; m /= p.Wq;
                const int hq = m % p.Hq; m /= p.Hq;
                const int tq = m % p.Tq; const int n = m / p.Tq;
                info = make_int4(n, tq * p.istr[0] + p.ioff0[0], hq * p.istr[1] + p.ioff0[1],
                                 wq * p.istr[2] + p.ioff0[2]);
                drow[c % 3][tid] = p.dlat ? ((n * p.Td + tq + p.doff[0]) * p.Hd + hq + p.doff[1]) * p.Wd + wq + p.doff[2] : pos;
            }
            ptab[c % 3][tid] = info;
        }
    };
    constexpr int DN = BK / DRP, SN = BK / SRP;        // loads per thread
    // tiles go global -> LDS directly (global_load_lds_dwordx4): each wave-instruction writes 1 KiB = consecutive
    // float4 columns of consecutive position rows, which is exactly the lane-linear image the DMA produces
    // (LDS float offset of thread tid in pass j = (tid + 256*j) * 4); invalid rows / taps read a zero line.
    // LDS-DMA through buffer resources (glds16b): the bases are the two tensors (wave-uniform), a lane's offset is 32-bit -- one 32-bit
    // multiply-add per piece instead of a 64-bit one and an address select; invalid rows / taps are DMA_OOB lanes (zero-filled)
    const dma_rsrc_t rsD = dma_rsrc(Dp + m0), rsS = dma_rsrc(Sp);
    const unsigned dcolb = mval ? (unsigned)dcol * 4u : DMA_OOB, csb = (unsigned)cs * 4u;
    auto gload = [&](int c, int buf) {
        float* ld = &Ds[buf][0][0] + wave * 256;      // wave-uniform base; the DMA adds lane*16 B
        float* ls = &Ss[buf][0][0] + wave * 256;
        if (ABL != 5)
#pragma unroll
        for (int j = 0; j < DN; ++j) {
            const int r = drow0 + DRP * j;
            const int pos = c * BK + r;
            const bool v = mval && pos < p.P;
            glds16b(rsD, v ? (unsigned)drow[c % 3][r] * (unsigned)(p.ldd * 4) + dcolb : DMA_OOB, ld + j * 1024);
        }
        if (ABL != 4)
#pragma unroll
        for (int j = 0; j < SN; ++j) {
            const int r = srow0 + SRP * j;
            const int4 info = ptab[c % 3][r];
            const int t = info.y + dt, h = info.z + dh, w = info.w + dw;
            const bool v = nval && info.x >= 0 && (unsigned)t < (unsigned)p.Ts && (unsigned)h < (unsigned)p.Hs &&
                           (unsigned)w < (unsigned)p.Ws;
            const unsigned ps = (unsigned)(((info.x * p.Ts + t) * p.Hs + h) * p.Ws + w);
            glds16b(rsS, v ? ps * (unsigned)(p.lds * 4) + csb : DMA_OOB, ls + j * 1024);
        }
    };

    f32x16 acc[TM][TN];
    f32x16 acc_lo[(X6 && HILO) ? TM : 1][(X6 && HILO) ? TN : 1];          // X6: `acc` takes the h*h products, acc_lo the five small ones (conv_x6.hip)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; if constexpr (X6 && HILO) acc_lo[i][j][r] = 0.f; }

    ptab_fill(c_begin);
    ptab_fill(c_begin + 1);
    __syncthreads();
    gload(c_begin, 0);
    PC_SYNC_DMA();
    const int ml = wm * (BM / 2) + (lane & 31), nl = wn * (BN / 2) + (lane & 31), kh = lane >> 5;
    for (int c = c_begin; c < c_end; ++c) {
        const int buf = (ABL >= 1 && ABL <= 3) ? 0 : ((c - c_begin) & 1);
        if (!ABL || ABL >= 4) ptab_fill(c + 2);
        if ((!ABL || ABL == 4 || ABL == 5) && c + 1 < c_end) gload(c + 1, buf ^ 1);   // 4: D tile only, 5: S tile only, 6: position table only
        if constexpr (X6) {
            static_assert(BK % 16 == 0 && ABL == 0, "whole k16 steps");
            typedef x6_u4 u4;
            auto load_split = [&](int s16, u4 (&A)[TM][3], u4 (&B)[TN][3]) {
                const int r0 = 16 * s16 + 8 * kh;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = Ds[buf][r0 + q][ml + i * 32];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { uint32_t h_, m_, l_; x6_split2(v[2 * q], v[2 * q + 1], h_, m_, l_); A[i][0][q] = h_; A[i][1][q] = m_; A[i][2][q] = l_; }
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) v[q] = Ss[buf][r0 + q][nl + j * 32];
#pragma unroll
                    for (int q = 0; q < 4; ++q) { uint32_t h_, m_, l_; x6_split2(v[2 * q], v[2 * q + 1], h_, m_, l_); B[j][0][q] = h_; B[j][1][q] = m_; B[j][2][q] = l_; }
                }
            };
            auto mma = [&](const u4 (&A)[TM][3], const u4 (&B)[TN][3]) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) x6_mma6(A[i], B[j], HILO ? acc_lo[HILO ? i : 0][HILO ? j : 0] : acc[i][j], acc[i][j]);
            };
            // (issuing the next step's reads and split in front of this step's MFMAs from a second register set, as wgrad3_x6_kernel does, was
            // measured on the 64 x 128 tile and bought nothing: 0.734 against 0.737 ms per step over its 19 launches -- two blocks per CU already
            // cover the split's latency)
#pragma unroll
            for (int s16 = 0; s16 < BK / 16; ++s16) {
                u4 A[TM][3], B[TN][3];
                load_split(s16, A, B);
                mma(A, B);
            }
        } else
#pragma unroll
        for (int ks = 0; ks < BK / 2; ++ks) {
            float af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = Ds[buf][(ABL >= 2 ? 0 : ks * 2) + kh][ml + i * 32];     // ABL >= 2: one read for the chunk
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = Ss[buf][(ABL >= 2 ? 0 : ks * 2) + kh][nl + j * 32];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        if (ABL < 3) PC_SYNC_DMA();        // the LDS-DMA of chunk c+1 has landed and the reads of chunk c are fenced
    }
    if constexpr (X6 && HILO) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] += acc_lo[i][j];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * (BM / 2) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= p.mend) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
                if (n < p.Ntot) {
                    // trimmed column (tap_local, cs) -> column of the full [KT*KH*KW][Cs] layout
                    const int tl = n / p.Cs, cc = n - tl * p.Cs;
                    const int ta = tl / tapHW, tr = tl - ta * tapHW, tb = tr / p.ntap[2], tc = tr - tb * p.ntap[2];
                    const int full = ((p.wk0[0] + ta) * p.KH + p.wk0[1] + tb) * p.KW + p.wk0[2] + tc;
                    float* dst = gp + (size_t)m * p.NtotFull + (size_t)full * p.Cs + cc;
                    if (p.store || p.wss) *dst = acc[i][j][r];
                    else atomicAdd(dst, acc[i][j][r]);
                }
            }
        }
}

template <int BM, int BN, int ABL = 0, int KB = 32>
__global__ __launch_bounds__(256, 2) void wgrad_kernel(const WgK p) {
    wgrad_body<BM, BN, ABL, KB>(p, xcd_remap(blockIdx.x, gridDim.x));
}
template <int BM, int BN, bool HILO = true>
__global__ __launch_bounds__(256, 2) void wgrad_x6_kernel(const WgK p) {
    wgrad_body<BM, BN, 0, 32, true, HILO>(p, xcd_remap(blockIdx.x, gridDim.x));
}

// Several weight-gradient problems in ONE grid (pc_conv_wgrad_multi): the wgrads of one Inception module, or the eight position
// classes of the merged tail.  Each problem keeps its own descriptor (by value in the kernel arguments) and a contiguous range of
// blocks sized in proportion to its work, so split-K fills the chip once per group instead of once per layer: fewer, longer K
// slices (a slice's 64 KB of atomics buy 4x the FLOPs) and no 30-microsecond launches for 1 GFLOP of work.
constexpr int WG_MAXJOBS = 8;
struct WgMulti { int njobs; int first[WG_MAXJOBS + 1]; WgK job[WG_MAXJOBS]; };

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void wgrad_multi_kernel(const WgMulti m) {
    int j = 0;
    const int bid = blockIdx.x;
    while (j + 1 < m.njobs && bid >= m.first[j + 1]) ++j;
    wgrad_body<BM, BN, 0, 32>(m.job[j], xcd_remap(bid - m.first[j], m.first[j + 1] - m.first[j]));
}


// Weight gradient of a conv with KW = 3 (padding 1) or 9 (no padding: the spectral forms' taps) taps of stride 1 along w
// (any stride along t / h) and Cs % 32 == 0: the K chunk is a segment of ONE image row, the column tile is (kw = 0..2) x 64 (or 32) channels of one (kt, kh)
// tap pair, and the KW taps read the SAME LDS tile of BKP + KW - 1 input positions at row offsets 0..KW-1 -- the
// gathered operand is fetched once per KW taps.  The generic kernel above is bound by the LDS-DMA fill of its two
// streaming operands; for the 64-channel layers this cuts the fill per FLOP by 1.8x.
struct Wg3K {
    const float* D; const float* S; float* g;
    int N, T, H, W, Cd, ldd, Cs, lds;
    int ntap_t, ntap_h, wk0_t, wk0_h, KH;     // (kt, kh) taps present (trimmed) and their place in the full [KT][KH][3] layout
    int Ts, Hs, istr_t, istr_h, ioff_t, ioff_h; // S row of output (t, h) and local tap (a, b): (t*istr_t + ioff_t + a, h*istr_h + ioff_h + b)
    int nseg, nchunks, chunks_per_split, nsplit, mt, ncs;   // segments per row; K chunks = N*T*H*nseg
    int taps_full;                            // KT*KH*KW: g is [Cd][taps_full][Cs]
    int Wsw, padw;                            // width of S and the padding along w (D width W = Wsw - KW + 1 + 2*padw)
    int nprob, store; long long dbs, sbs, gbs; // independent problems in one launch (pointer strides); plain stores (one K slice)
    long long wss;                            // > 0: K-slice images in a workspace instead of atomics (WgK::wss)
};

template <int BM, int BKP, int CSB, int WMW, int KW = 3>
__global__ __launch_bounds__(256, 2) void wgrad3_kernel(const Wg3K p) {
    constexpr int BN = KW * CSB, WNW = 4 / WMW;                            // WMW x WNW waves
    constexpr int TM = BM / WMW / 32, TN = BN / WNW / 32;
    static_assert(BM % (WMW * 32) == 0 && BN % (WNW * 32) == 0, "wave tiles");
    constexpr int SPIECE = 256 / CSB;                                      // S rows per 1 KiB DMA piece
    constexpr int SROWS = (BKP + KW - 1 + SPIECE - 1) / SPIECE * SPIECE;   // S tile rows padded to whole DMA pieces
    constexpr int DI = BKP * BM * 4 / 1024, SI = SROWS * CSB * 4 / 1024;   // DMA wave-instructions per tile
    static_assert((BKP * BM * 4) % 1024 == 0, "D tile must be whole DMA pieces");
    // One LDS variable per ring slot and the slot a compile-time constant (the chunk loop is unrolled by two): the compiler's
    // s_waitcnt pass orders every LDS read behind every in-flight LDS-DMA write it cannot prove disjoint, and it can only prove it
    // for distinct variables.  With Ds[2][..] indexed by a run-time slot it put s_waitcnt vmcnt(0) between the fetch of chunk c + 1
    // and the first operand read of chunk c -- the fetch was never in flight during the MFMA loop (MFMA busy 0.61).
    __shared__ __attribute__((aligned(16))) float Ds0[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ds1[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ss0[SROWS][CSB];
    __shared__ __attribute__((aligned(16))) float Ss1[SROWS][CSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = p.mt * p.ncs * p.ntap_t * p.ntap_h;
    int tile = lid % tiles;
    const int slice = (lid / tiles) % p.nsplit, prob = lid / (tiles * p.nsplit);
    const float* Dp = p.D + (size_t)prob * p.dbs;
    const float* Sp = p.S + (size_t)prob * p.sbs;
    float* gp = p.g + (size_t)prob * p.gbs + (size_t)slice * p.wss;
    const int mtile = tile % p.mt; tile /= p.mt;
    const int csb = tile % p.ncs; tile /= p.ncs;
    const int kh_ = tile % p.ntap_h, kt_ = tile / p.ntap_h;
    const int m0 = mtile * BM, cs0 = csb * CSB;
    const int c_begin = slice * p.chunks_per_split, c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    if (c_begin >= c_end) return;

    // chunk -> (n, t, h, seg), kept as a counter that advances with every fetch (chunks are fetched in order: no divisions in the
    // K loop); a fetch returns false when the tap pair reads outside the volume (the chunk contributes nothing)
    int q_seg = c_begin % p.nseg, q_h, q_t, q_n;
    { int r = c_begin / p.nseg; q_h = r % p.H; r /= p.H; q_t = r % p.T; q_n = r / p.T; }
    auto decode = [&](int& row_d, int& row_s, int& w0) -> bool {
        w0 = q_seg * BKP;
        row_d = ((q_n * p.T + q_t) * p.H + q_h) * p.W;
        const int ts = q_t * p.istr_t + p.ioff_t + kt_, hs = q_h * p.istr_h + p.ioff_h + kh_;
        row_s = ((q_n * p.Ts + ts) * p.Hs + hs) * p.Wsw;
        if (++q_seg == p.nseg) { q_seg = 0; if (++q_h == p.H) { q_h = 0; if (++q_t == p.T) { q_t = 0; ++q_n; } } }
        return (unsigned)ts < (unsigned)p.Ts && (unsigned)hs < (unsigned)p.Hs;
    };
    auto gload = [&](auto slot) -> bool {
        constexpr int buf = decltype(slot)::value;
        int row_d, row_s, w0;
        if (!decode(row_d, row_s, w0)) return false;
        float* ld = buf ? &Ds1[0][0] : &Ds0[0][0];
        float* ls = buf ? &Ss1[0][0] : &Ss0[0][0];
        // wave-uniform bases: the segment's first position (the S base may lie padw positions in front of its row: only address arithmetic)
        const dma_rsrc_t rsD = dma_rsrc(Dp + (size_t)(row_d + w0) * p.ldd + m0);
        const dma_rsrc_t rsS = dma_rsrc(Sp + ((long long)row_s + w0 - p.padw) * p.lds + cs0);
#pragma unroll
        for (int jj = 0; jj < (DI + 3) / 4; ++jj) {                        // D tile: BKP rows x BM channels
            const int i = jj * 4 + wave;
            if (i >= DI) break;
            const int e = i * 64 + lane, r = e / (BM / 4), c4 = e % (BM / 4);
            const bool v = (w0 + r) < p.W && (m0 + c4 * 4) < p.Cd;
            glds16b(rsD, v ? (unsigned)(r * p.ldd + c4 * 4) * 4u : DMA_OOB, ld + i * 256);
        }
#pragma unroll
        for (int jj = 0; jj < (SI + 3) / 4; ++jj) {                        // S tile: positions w0-pad .. w0-pad+BKP+KW-2 (+ padding rows)
            const int i = jj * 4 + wave;
            if (i >= SI) break;
            const int e = i * 64 + lane, r = e / (CSB / 4), c4 = e % (CSB / 4);
            const int w = w0 - p.padw + r;
            const bool v = r < BKP + KW - 1 && (unsigned)w < (unsigned)p.Wsw;
            glds16b(rsS, v ? (unsigned)(r * p.lds + c4 * 4) * 4u : DMA_OOB, ls + i * 256);
        }
        return true;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // column tile j of wave wn: columns wn*96 + 32j .. +31 of (kw, cs): kw = col / 64, cs = col % 64
    int kwj[TN], csj[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int col = wn * (BN / WNW) + 32 * j; kwj[j] = col / CSB; csj[j] = col % CSB + (lane & 31); }
    const int ml = wm * (BM / WMW) + (lane & 31), kh = lane >> 5;
    bool live = gload(std::integral_constant<int, 0>{});
    PC_SYNC_DMA();
    auto chunk = [&](auto slot, int c) {
        constexpr int buf = decltype(slot)::value;
        const bool next_live = c + 1 < c_end ? gload(std::integral_constant<int, buf ^ 1>{}) : false;
        if (live) {
            const float (*Dt)[BM] = buf ? Ds1 : Ds0;
            const float (*St)[CSB] = buf ? Ss1 : Ss0;
#pragma unroll
            for (int ks = 0; ks < BKP / 2; ++ks) {
                const int pp = ks * 2 + kh;
                float af[TM], bf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) af[i] = Dt[pp][ml + i * 32];
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[j] = St[pp + kwj[j]][csj[j]];
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
            }
        }
        PC_SYNC_DMA();        // the LDS-DMA of chunk c+1 has landed and the reads of chunk c are fenced
        live = next_live;
    };
    for (int c = c_begin; c < c_end; c += 2) {
        chunk(std::integral_constant<int, 0>{}, c);
        if (c + 1 < c_end) chunk(std::integral_constant<int, 1>{}, c + 1);
    }
    const int tapbase = ((kt_ + p.wk0_t) * p.KH + kh_ + p.wk0_h) * KW;    // + kw
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * (BM / WMW) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= p.Cd) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float* dst = gp + ((size_t)m * p.taps_full + tapbase + kwj[j]) * p.Cs + cs0 + csj[j];
                if (p.store || p.wss) *dst = acc[i][j][r];
                else atomicAdd(dst, acc[i][j][r]);
            }
        }
}



// ---- the same row-segment weight gradient with the multiplications on the bf16 matrix cores (csrc/conv_x6.hip has the scheme: three bf16
// terms per fp32 operand, six products, hi / lo accumulators).  Both operands are activations here, so both are split in registers: a lane's
// operand of v_mfma_f32_32x32x16_bf16 is eight consecutive POSITIONS of one channel -- eight ds_read_b32 down a column of the [position]
// [channel] tile the LDS-DMA left (conflict-free: a half-wave reads 32 consecutive channels of one row) -- and the KW = 3 taps share them:
// the ten source values at positions 8 g .. 8 g + 9 are read and split ONCE, tap 0 takes the packed pairs 0..3, tap 2 the pairs 1..4, tap 1
// re-pairs them with four v_alignbit per plane.  Per k16 step and wave: 18 reads + 111 vector instructions beside 18 MFMAs.
// One 32-channel tile of D and one 32-channel half of S per wave (all three taps): BM = 32 WMW, CSB = 32 (4 / WMW).  BKP (a multiple of
// 16) positions per chunk; a segment that runs past the row end reads zeros (LDS-DMA out-of-range lanes).
// (two ring slots of more than 80 KiB -- BM = 128 with BKP = 64: 82 KiB -- admit one block per CU, and the launch bound says so: the same code
// as with a bound of two, which the compiler could not meet and warned about)
template <int BM, int BKP, int CSB, int WMW>
__global__ __launch_bounds__(256, 2 * (BKP * BM + (BKP + 8) * CSB) * 4 > 80 * 1024 ? 1 : 2) void wgrad3_x6_kernel(const Wg3K p) {
    constexpr int KW = 3, WNW = 4 / WMW, NS = BKP / 16;
    static_assert(BM == 32 * WMW && CSB == 32 * WNW && BKP % 16 == 0, "one 32-channel tile of D and of S per wave");
    constexpr int SPIECE = 256 / CSB;
    constexpr int SROWS = (BKP + KW - 1 + SPIECE - 1) / SPIECE * SPIECE;
    constexpr int DI = BKP * BM * 4 / 1024, SI = SROWS * CSB * 4 / 1024;
    static_assert((BKP * BM * 4) % 1024 == 0, "D tile must be whole DMA pieces");
    __shared__ __attribute__((aligned(16))) float Ds0[BKP][BM];          // one variable per ring slot: see wgrad3_kernel
    __shared__ __attribute__((aligned(16))) float Ds1[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ss0[SROWS][CSB];
    __shared__ __attribute__((aligned(16))) float Ss1[SROWS][CSB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNW, wn = wave % WNW;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = p.mt * p.ncs * p.ntap_t * p.ntap_h;
    int tile = lid % tiles;
    const int slice = (lid / tiles) % p.nsplit, prob = lid / (tiles * p.nsplit);
    const float* Dp = p.D + (size_t)prob * p.dbs;
    const float* Sp = p.S + (size_t)prob * p.sbs;
    float* gp = p.g + (size_t)prob * p.gbs + (size_t)slice * p.wss;
    const int mtile = tile % p.mt; tile /= p.mt;
    const int csb = tile % p.ncs; tile /= p.ncs;
    const int kh_ = tile % p.ntap_h, kt_ = tile / p.ntap_h;
    const int m0 = mtile * BM, cs0 = csb * CSB;
    const int c_begin = slice * p.chunks_per_split, c_end = min(p.nchunks, c_begin + p.chunks_per_split);
    if (c_begin >= c_end) return;

    int q_seg = c_begin % p.nseg, q_h, q_t, q_n;
    { int r = c_begin / p.nseg; q_h = r % p.H; r /= p.H; q_t = r % p.T; q_n = r / p.T; }
    auto decode = [&](int& row_d, int& row_s, int& w0) -> bool {
        w0 = q_seg * BKP;
        row_d = ((q_n * p.T + q_t) * p.H + q_h) * p.W;
        const int ts = q_t * p.istr_t + p.ioff_t + kt_, hs = q_h * p.istr_h + p.ioff_h + kh_;
        row_s = ((q_n * p.Ts + ts) * p.Hs + hs) * p.Wsw;
        if (++q_seg == p.nseg) { q_seg = 0; if (++q_h == p.H) { q_h = 0; if (++q_t == p.T) { q_t = 0; ++q_n; } } }
        return (unsigned)ts < (unsigned)p.Ts && (unsigned)hs < (unsigned)p.Hs;
    };
    auto gload = [&](auto slot) -> bool {
        constexpr int buf = decltype(slot)::value;
        int row_d, row_s, w0;
        if (!decode(row_d, row_s, w0)) return false;
        float* ld = buf ? &Ds1[0][0] : &Ds0[0][0];
        float* ls = buf ? &Ss1[0][0] : &Ss0[0][0];
        const dma_rsrc_t rsD = dma_rsrc(Dp + (size_t)(row_d + w0) * p.ldd + m0);
        const dma_rsrc_t rsS = dma_rsrc(Sp + ((long long)row_s + w0 - p.padw) * p.lds + cs0);
#pragma unroll
        for (int jj = 0; jj < (DI + 3) / 4; ++jj) {
            const int i = jj * 4 + wave;
            if (i >= DI) break;
            const int e = i * 64 + lane, r = e / (BM / 4), c4 = e % (BM / 4);
            const bool v = (w0 + r) < p.W && (m0 + c4 * 4) < p.Cd;                   // past the row end: zeros
            glds16b(rsD, v ? (unsigned)(r * p.ldd + c4 * 4) * 4u : DMA_OOB, ld + i * 256);
        }
#pragma unroll
        for (int jj = 0; jj < (SI + 3) / 4; ++jj) {
            const int i = jj * 4 + wave;
            if (i >= SI) break;
            const int e = i * 64 + lane, r = e / (CSB / 4), c4 = e % (CSB / 4);
            const int w = w0 - p.padw + r;
            const bool v = r < BKP + KW - 1 && (unsigned)w < (unsigned)p.Wsw;
            glds16b(rsS, v ? (unsigned)(r * p.lds + c4 * 4) * 4u : DMA_OOB, ls + i * 256);
        }
        return true;
    };

    f32x16 acc_hi[KW], acc_lo[KW];
#pragma unroll
    for (int j = 0; j < KW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_hi[j][r] = 0.f; acc_lo[j][r] = 0.f; }
    const int ml = wm * 32 + (lane & 31), csl = wn * 32 + (lane & 31), kg = lane >> 5;
    typedef uint32_t u32;
    // planes of one k16 step: A (D^T) [plane][4 regs]; B pairs p = 0..4 of the ten source values [plane][5]
    auto load_split = [&](const float (*Dt)[BM], const float (*St)[CSB], int s, u32 (&pa)[3][4], u32 (&pb)[3][5]) {
        const int r0 = 16 * s + 8 * kg;
        float a[8], b[10];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = Dt[r0 + j][ml];
#pragma unroll
        for (int j = 0; j < 10; ++j) b[j] = St[r0 + j][csl];
#pragma unroll
        for (int q = 0; q < 4; ++q) x6_split2(a[2 * q], a[2 * q + 1], pa[0][q], pa[1][q], pa[2][q]);
#pragma unroll
        for (int q = 0; q < 5; ++q) x6_split2(b[2 * q], b[2 * q + 1], pb[0][q], pb[1][q], pb[2][q]);
    };
    typedef x6_u4 u4;
    auto mma_step = [&](const u32 (&pa)[3][4], const u32 (&pb)[3][5]) {
        u4 A[3], B[KW][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            A[pl] = u4{pa[pl][0], pa[pl][1], pa[pl][2], pa[pl][3]};
            B[0][pl] = u4{pb[pl][0], pb[pl][1], pb[pl][2], pb[pl][3]};
            B[2][pl] = u4{pb[pl][1], pb[pl][2], pb[pl][3], pb[pl][4]};
            // tap 1: positions 1..8 = (hi of pair q, lo of pair q + 1)
            B[1][pl] = u4{__builtin_amdgcn_alignbit(pb[pl][1], pb[pl][0], 16), __builtin_amdgcn_alignbit(pb[pl][2], pb[pl][1], 16),
                          __builtin_amdgcn_alignbit(pb[pl][3], pb[pl][2], 16), __builtin_amdgcn_alignbit(pb[pl][4], pb[pl][3], 16)};
        }
#pragma unroll
        for (int j = 0; j < KW; ++j) x6_mma6(A, B[j], acc_lo[j], acc_hi[j]);
    };
    bool live = gload(std::integral_constant<int, 0>{});
    PC_SYNC_DMA();
    auto chunk = [&](auto slot, int c) {
        constexpr int buf = decltype(slot)::value;
        const bool next_live = c + 1 < c_end ? gload(std::integral_constant<int, buf ^ 1>{}) : false;
        if (live) {
            const float (*Dt)[BM] = buf ? Ds1 : Ds0;
            const float (*St)[CSB] = buf ? Ss1 : Ss0;
            u32 pa[2][3][4], pb[2][3][5];
            load_split(Dt, St, 0, pa[0], pb[0]);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (s + 1 < NS) load_split(Dt, St, s + 1, pa[(s + 1) & 1], pb[(s + 1) & 1]);      // the next step's reads and split beside this step's MFMAs
                mma_step(pa[s & 1], pb[s & 1]);
            }
        }
        PC_SYNC_DMA();        // the LDS-DMA of chunk c+1 has landed and the reads of chunk c are fenced
        live = next_live;
    };
    for (int c = c_begin; c < c_end; c += 2) {
        chunk(std::integral_constant<int, 0>{}, c);
        if (c + 1 < c_end) chunk(std::integral_constant<int, 1>{}, c + 1);
    }
    const int tapbase = ((kt_ + p.wk0_t) * p.KH + kh_ + p.wk0_h) * KW;    // + kw
#pragma unroll
    for (int j = 0; j < KW; ++j) {
        const f32x16 acc = acc_hi[j] + acc_lo[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m >= p.Cd) continue;
            float* dst = gp + ((size_t)m * p.taps_full + tapbase + j) * p.Cs + cs0 + csl;
            if (p.store || p.wss) *dst = acc[r];
            else atomicAdd(dst, acc[r]);
        }
    }
}


// ---- weight gradient of a 4-channel source with stride SW along w (the stem: 7x7x7, stride 2, 3 channels padded to 4) --------
// One tap of 4 channels is one 16-byte piece, so the generic kernel gathers its S tile piece by piece (64 taps x 16 positions
// = 1024 pieces per chunk, each input piece fetched ~3x per chunk).  Here the K chunk is a segment of BKP positions of ONE
// output row, and a block owns ALL (kh, kw) taps of one kt: per kh one LDS row of SW*BKP + KW - 1 input pieces, fetched once.
// Column n = kw*4 + cs of tap row kh for position k is LDS dword kh*ROW + 4*SW*k + n: 32 consecutive dwords per MFMA operand,
// conflict-free.  (kw = KW..7 are padding columns, dropped at the store.)  Waves: 2 halves of the 64 channels of D x 2 k-step
// parities, 7 (= KH) 32x32 accumulators each.  Chunks whose kt tap reads outside the volume along t are not enumerated at all,
// and the K slices are dealt to the kt taps in proportion to their valid chunks.
struct Wg4K {
    const float* D; const float* S; float* g;
    int N, T, H, W, Cd, ldd, lds;
    int ntap_t, wk0_t, wk0_h, KH;
    int Ts, Hs, Wsw, istr_t, istr_h, ioff_t, ioff_h, padw;
    int nseg, mt, taps_full;
    int pre[11];                               // slice prefix per kt (ntap_t + 1 entries)
    int interleave;                            // 1: order[] below is valid
    long long wss;                             // > 0: K-slice images in a workspace instead of atomics (WgK::wss); image index = slice within its kt
    unsigned short order[1024];                // block q of an m tile -> slice index (kt slices interleaved by their position in the volume)
};

// PACK3 (PC_WG_CS3: the 4th source channel is padding): the NKH * KW * 3 real columns are packed into ceil(147 / 32) = 5
// accumulators instead of one 32-column accumulator per kh with 21 real columns in it -- 5 MFMAs per k-step instead of 7.  Column
// G = jj * 32 + lane -> (kh, kw, cs) = (G / 21, G % 21 / 3, G % 3) reads LDS dword kh*ROW + 4*SW*k + 4*kw + cs: per-lane constant
// offsets; the padding dwords leave a quarter of the banks unused, so these ds_read_b32 are 2-way conflicted (2 of 22 LDS cycles
// per k-step more per wave, far from the LDS limit).
template <int BKP, int KW, int SW, int NKH, bool PACK3>
__global__ __launch_bounds__(256, 2) void wgrad4_kernel(const Wg4K p) {
    constexpr int BM = 64;
    constexpr int ROWP = SW * BKP + KW - 1;                  // pieces per kh row
    static_assert(SW * (BKP - 1) + 7 < ROWP + 1, "padding columns stay inside the row");
    constexpr int SPIECES = NKH * ROWP, SI = (SPIECES + 63) / 64, DI = BKP * BM * 4 / 1024;
    static_assert((BKP * BM * 4) % 1024 == 0 && (BKP / 2) % 2 == 0, "tile shape");
    __shared__ __attribute__((aligned(16))) float Ds0[BKP][BM];          // one variable per ring slot: see wgrad3_kernel
    __shared__ __attribute__((aligned(16))) float Ds1[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ss0[SI * 256];
    __shared__ __attribute__((aligned(16))) float Ss1[SI * 256];
    __shared__ float xch[2][16][64];                                     // epilogue of the K-slice-image form: wave wk = 1 -> wave wk = 0
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wk = wave >> 1;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    // The slices of the seven kt taps that cover the same stretch of the volume read the same D rows: they sit next to each other in block order
    // (one XCD, one moment), so those rows come out of L2 instead of HBM seven times (1.6 GB per launch for 0.31 GB of operands before)
    const int mtile = lid % p.mt, sl = p.interleave ? (int)p.order[lid / p.mt] : lid / p.mt;
    int kt_ = 0;
    while (kt_ + 1 < p.ntap_t && sl >= p.pre[kt_ + 1]) ++kt_;
    const int slice = sl - p.pre[kt_], nsplit = p.pre[kt_ + 1] - p.pre[kt_];
    // output t with a valid source t for this tap
    int tlo = 0, thi = p.T - 1;
    while (tlo <= thi && tlo * p.istr_t + p.ioff_t + kt_ < 0) ++tlo;
    while (thi >= tlo && thi * p.istr_t + p.ioff_t + kt_ >= p.Ts) --thi;
    const int ntv = thi - tlo + 1;
    const int nchunks = p.N * ntv * p.H * p.nseg;
    const int cps = (nchunks + nsplit - 1) / nsplit;
    const int c_begin = slice * cps, c_end = min(nchunks, c_begin + cps);
    if (c_begin >= c_end) return;
    const int m0 = mtile * BM;

    // chunk -> (n, t, h, seg) as a counter advanced by every fetch (chunks are fetched in order)
    int q_seg = c_begin % p.nseg, q_h, q_t, q_n;
    { int r = c_begin / p.nseg; q_h = r % p.H; r /= p.H; q_t = r % ntv; q_n = r / ntv; }
    auto gload = [&](auto slot) {
        constexpr int buf = decltype(slot)::value;
        const int seg = q_seg, h = q_h, t = tlo + q_t, n = q_n;
        if (++q_seg == p.nseg) { q_seg = 0; if (++q_h == p.H) { q_h = 0; if (++q_t == ntv) { q_t = 0; ++q_n; } } }
        const int w0 = seg * BKP;
        const int row_d = ((n * p.T + t) * p.H + h) * p.W;
        const int ts = t * p.istr_t + p.ioff_t + kt_, hs0 = h * p.istr_h + p.ioff_h;
        float* ld = buf ? &Ds1[0][0] : &Ds0[0][0];
        float* ls = buf ? &Ss1[0] : &Ss0[0];
        const dma_rsrc_t rsD = dma_rsrc(p.D + (size_t)(row_d + w0) * p.ldd + m0);
        // S rows hs0 .. hs0 + NKH - 1 of frame (n, ts), from w0*SW - padw on: base at (hs0, w0*SW - padw) -- possibly in front of the frame
        const dma_rsrc_t rsS = dma_rsrc(p.S + (((long long)(n * p.Ts + ts) * p.Hs + hs0) * p.Wsw + (long long)w0 * SW - p.padw) * p.lds);
#pragma unroll
        for (int jj = 0; jj < (DI + 3) / 4; ++jj) {
            const int i = jj * 4 + wave;
            if (i >= DI) break;
            const int e = i * 64 + lane, rr = e / (BM / 4), c4 = e % (BM / 4);
            const bool v = (m0 + c4 * 4) < p.Cd;
            glds16b(rsD, v ? (unsigned)(rr * p.ldd + c4 * 4) * 4u : DMA_OOB, ld + i * 256);
        }
#pragma unroll
        for (int jj = 0; jj < (SI + 3) / 4; ++jj) {
            const int i = jj * 4 + wave;
            if (i >= SI) break;
            const int e = i * 64 + lane, kh = e / ROWP, rr = e - kh * ROWP;
            const int hs = hs0 + kh, w = w0 * SW - p.padw + rr;
            const bool v = kh < NKH && (unsigned)hs < (unsigned)p.Hs && (unsigned)w < (unsigned)p.Wsw;
            glds16b(rsS, v ? (unsigned)((kh * p.Wsw + rr) * p.lds) * 4u : DMA_OOB, ls + i * 256);     
        }
    };

    constexpr int NCOL = NKH * KW * 3, NACC = PACK3 ? (NCOL + 31) / 32 : NKH;
    f32x16 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const int nl = lane & 31, kh2 = lane >> 5, ml = wm * 32 + nl;
    int boff[NACC], gcol[NACC];                // LDS dword of this lane's column in accumulator j / its offset inside g's [tap][4] rows (-1: none)
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        if constexpr (PACK3) {
            const int G = j * 32 + nl, kh = G / (KW * 3), rem = G - kh * (KW * 3), kw = rem / 3, cs = rem - kw * 3;
            const bool v = G < NCOL;
            boff[j] = v ? kh * ROWP * 4 + kw * 4 + cs : 0;
            gcol[j] = v ? (kh * KW + kw) * 4 + cs : -1;
        } else {
            boff[j] = j * ROWP * 4 + nl;
            gcol[j] = nl < KW * 4 ? j * KW * 4 + nl : -1;          // kw = KW..7 are padding columns
        }
    }
    gload(std::integral_constant<int, 0>{});
    PC_SYNC_DMA();
    auto chunk = [&](auto slot, int c) {
        constexpr int buf = decltype(slot)::value;
        if (c + 1 < c_end) gload(std::integral_constant<int, buf ^ 1>{});
        const float* sb = buf ? &Ss1[0] : &Ss0[0];
        const float (*Dt)[BM] = buf ? Ds1 : Ds0;
#pragma unroll
        for (int q = 0; q < BKP / 4; ++q) {
            const int pp = (2 * q + wk) * 2 + kh2;
            const float af = Dt[pp][ml];
            float bf[NACC];
#pragma unroll
            for (int j = 0; j < NACC; ++j) bf[j] = sb[boff[j] + 4 * SW * pp];
#pragma unroll
            for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf[j], acc[j], 0, 0, 0);
        }
        PC_SYNC_DMA();
    };
    for (int c = c_begin; c < c_end; c += 2) {
        chunk(std::integral_constant<int, 0>{}, c);
        if (c + 1 < c_end) chunk(std::integral_constant<int, 1>{}, c + 1);
    }
    const size_t tap0 = (size_t)((kt_ + p.wk0_t) * p.KH + p.wk0_h) * KW * 4;       // g offset of (kt, kh = 0, kw = 0, cs = 0)
    if (p.wss) {
        // K-slice image instead of atomics: the two k-step parities (waves wk = 0 / 1) hold partial sums of the SAME outputs, which the atomics
        // used to combine -- here wave wk = 1 hands its accumulators to wave wk = 0 through LDS (one accumulator per round), which adds them in a
        // fixed order and stores the image with plain stores
        float* image = p.g + (size_t)slice * p.wss;
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            if (wk == 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) xch[wm][r][lane] = acc[j][r];
            }
            __syncthreads();
            if (wk == 0 && gcol[j] >= 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < p.Cd) image[(size_t)m * p.taps_full * 4 + tap0 + gcol[j]] = acc[j][r] + xch[wm][r][lane];
                }
            }
            __syncthreads();
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= p.Cd) continue;
#pragma unroll
        for (int j = 0; j < NACC; ++j)
            if (gcol[j] >= 0) atomicAdd(p.g + (size_t)m * p.taps_full * 4 + tap0 + gcol[j], acc[j][r]);
    }
}

// ---- the stem's weight gradient on the bf16 matrix cores (round 6; conv_x6.hip has the scheme: three bf16 terms per fp32 operand, six products,
// hi / lo accumulators).  Same problem and LDS images as wgrad4_kernel<.., PACK3> -- a block owns all 7 x 7 (kh, kw) taps x 3 real source channels
// of one kt, packed into five 32-column accumulators; every input piece is fetched once per chunk -- but the K chunk is TWO sub-chunks of 16
// consecutive output positions of a row (112 = 7 x 16: no padding positions, where 28-position segments would leave 4 of 32 empty), one k16
// step each: waves = 2 halves of D's 64 channels x the 2 sub-chunks.  Both operands are activations, so both are split in registers: a lane's
// MFMA operand is eight consecutive POSITIONS of one column -- eight ds_read_b32 down the D tile, eight ds_read_b32 eight dwords apart (SW * 4)
// along an input row for (kh, kw, cs).  Per wave and chunk: 48 LDS reads, 24 two-element splits, 30 MFMAs -- 0.6 microseconds of matrix-pipe
// time, less than the latency of an LDS-DMA fetch: the tiles live in a THREE-deep ring (chunk c + 2 is fetched while chunk c is multiplied) with
// counted waits (every wave issues the same five DMA instructions per chunk, so "chunk c has landed" is vmcnt <= 5 while chunk c + 1 is in flight).
template <int KW, int SW, int NKH>
__global__ __launch_bounds__(256, 2) void wgrad4_x6_kernel(const Wg4K p) {
    constexpr int BM = 64, SUB = 16, BKP = 2 * SUB;
    constexpr int ROWP = SW * SUB + KW - 1;                  // pieces per kh row of a sub-chunk
    constexpr int SPIECES = NKH * ROWP, SI = 6, SSUB = SI * 256, DI = BKP * BM * 4 / 1024;     // six DMA instructions per sub-chunk image (the last two partly / all padding)
    constexpr int NCOL = NKH * KW * 3, NACC = (NCOL + 31) / 32;
    constexpr int NDMA = 5;                                  // DMA instructions per wave and chunk: 2 of D, 3 of S
    static_assert(DI == 8 && SPIECES <= SI * 64 && 2 * SI == 12, "tile shape");
    __shared__ __attribute__((aligned(16))) float Ds0[BKP][BM];          // one variable per ring slot: see wgrad3_kernel
    __shared__ __attribute__((aligned(16))) float Ds1[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ds2[BKP][BM];
    __shared__ __attribute__((aligned(16))) float Ss0[2 * SSUB];
    __shared__ __attribute__((aligned(16))) float Ss1[2 * SSUB];
    __shared__ __attribute__((aligned(16))) float Ss2[2 * SSUB];
    __shared__ float xch[2][16][64];                                     // epilogue: wave wk = 1 -> wave wk = 0
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wk = wave >> 1;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int mtile = lid % p.mt, sl = p.interleave ? (int)p.order[lid / p.mt] : lid / p.mt;
    int kt_ = 0;
    while (kt_ + 1 < p.ntap_t && sl >= p.pre[kt_ + 1]) ++kt_;
    const int slice = sl - p.pre[kt_], nsplit = p.pre[kt_ + 1] - p.pre[kt_];
    int tlo = 0, thi = p.T - 1;
    while (tlo <= thi && tlo * p.istr_t + p.ioff_t + kt_ < 0) ++tlo;
    while (thi >= tlo && thi * p.istr_t + p.ioff_t + kt_ >= p.Ts) --thi;
    const int ntv = thi - tlo + 1;
    const int nsub = p.N * ntv * p.H * p.nseg;               // sub-chunks (p.nseg = ceil(W / 16) per row)
    const int nchunks = (nsub + 1) / 2;
    const int cps = (nchunks + nsplit - 1) / nsplit;
    const int c_begin = slice * cps, c_end = min(nchunks, c_begin + cps);
    if (c_begin >= c_end) return;
    const int m0 = mtile * BM;

    // sub-chunk -> (n, t, h, seg) as a counter advanced by every fetch (two sub-chunks per chunk, in order)
    int q_seg, q_h, q_t, q_n, q_idx = 2 * c_begin;
    { int r = q_idx; q_seg = r % p.nseg; r /= p.nseg; q_h = r % p.H; r /= p.H; q_t = r % ntv; q_n = r / ntv; }
    auto gload = [&](auto slot) {
        constexpr int buf = decltype(slot)::value;
        float* ld = buf == 0 ? &Ds0[0][0] : buf == 1 ? &Ds1[0][0] : &Ds2[0][0];
        float* ls = buf == 0 ? &Ss0[0] : buf == 1 ? &Ss1[0] : &Ss2[0];
        dma_rsrc_t rsS[2];
        int hs0_[2], w0_[2]; bool live_[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const bool live = q_idx < nsub;                   // an odd number of sub-chunks: the last chunk's second half reads zeros
            const int seg = q_seg, h = q_h, t = tlo + q_t, n = q_n;
            ++q_idx;
            if (++q_seg == p.nseg) { q_seg = 0; if (++q_h == p.H) { q_h = 0; if (++q_t == ntv) { q_t = 0; ++q_n; } } }
            const int w0 = seg * SUB;
            const int row_d = ((n * p.T + t) * p.H + h) * p.W;
            const int ts = t * p.istr_t + p.ioff_t + kt_, hs0 = h * p.istr_h + p.ioff_h;
            const dma_rsrc_t rsD = dma_rsrc(p.D + (live ? (size_t)(row_d + w0) * p.ldd + m0 : 0));
            rsS[sub] = dma_rsrc(p.S + (live ? (((long long)(n * p.Ts + ts) * p.Hs + hs0) * p.Wsw + (long long)w0 * SW - p.padw) * p.lds : 0));
            hs0_[sub] = hs0; w0_[sub] = w0; live_[sub] = live;
            {   // D: DMA instruction sub * 4 + wave = rows 16 sub + 4 wave .. + 3 of the chunk's tile
                const int i = sub * 4 + wave;
                const int rr = lane >> 4, c4 = lane & 15, r16 = wave * 4 + rr;
                const bool v = live && (w0 + r16) < p.W && (m0 + c4 * 4) < p.Cd;
                glds16b(rsD, v ? (unsigned)(r16 * p.ldd + c4 * 4) * 4u : DMA_OOB, ld + i * 256);
            }
        }
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) {                      // S: instruction wave + 4 jj of the chunk's twelve: sub-chunk image i / 6, its piece row i % 6
            const int i = jj * 4 + wave, sub = i / SI, ii = i - sub * SI;
            const int e = ii * 64 + lane, kh = e / ROWP, rr = e - kh * ROWP;
            const int hs = hs0_[sub] + kh, w = w0_[sub] * SW - p.padw + rr;
            const bool v = live_[sub] && kh < NKH && (unsigned)hs < (unsigned)p.Hs && (unsigned)w < (unsigned)p.Wsw;
            glds16b(rsS[sub], v ? (unsigned)((kh * p.Wsw + rr) * p.lds) * 4u : DMA_OOB, ls + i * 256);
        }
    };

    f32x16 acc_hi[NACC], acc_lo[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc_hi[j][r] = 0.f; acc_lo[j][r] = 0.f; }
    const int nl = lane & 31, kg = lane >> 5, ml = wm * 32 + nl;
    int boff[NACC], gcol[NACC];                // LDS dword of this lane's column in accumulator j at its first position / its offset inside g's [tap][4] rows (-1: none)
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int G = j * 32 + nl, kh = G / (KW * 3), rem = G - kh * (KW * 3), kw = rem / 3, cs = rem - kw * 3;
        const bool v = G < NCOL;
        boff[j] = (v ? kh * ROWP * 4 + kw * 4 + cs : 0) + wk * SSUB + 4 * SW * 8 * kg;
        gcol[j] = v ? (kh * KW + kw) * 4 + cs : -1;
    }
    typedef x6_u4 u4;
    auto chunk = [&](auto slot, int c) {
        constexpr int buf = decltype(slot)::value;
        // chunk c has landed for every wave (counted: chunk c + 1, if any, stays in flight) and every wave is done with chunk c - 1, whose slot
        // the fetch of chunk c + 2 overwrites.  The waits are written out (PC_SYNC_DMA, common.h: the compiler's own bookkeeping lost them once)
        if (c + 1 < c_end) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (c + 2 < c_end) gload(std::integral_constant<int, (buf + 2) % 3>{});
        const float* sb = buf == 0 ? &Ss0[0] : buf == 1 ? &Ss1[0] : &Ss2[0];
        const float (*Dt)[BM] = buf == 0 ? Ds0 : buf == 1 ? Ds1 : Ds2;
        u4 A[3];
        {
            float a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = Dt[wk * SUB + 8 * kg + q][ml];
#pragma unroll
            for (int q = 0; q < 4; ++q) { uint32_t h_, m_, l_; x6_split2(a[2 * q], a[2 * q + 1], h_, m_, l_); A[0][q] = h_; A[1][q] = m_; A[2][q] = l_; }
        }
        float b[NACC][8];
#pragma unroll
        for (int j = 0; j < NACC; ++j)
#pragma unroll
            for (int q = 0; q < 8; ++q) b[j][q] = sb[boff[j] + 4 * SW * q];
        // software pipeline inside the chunk: the split of column tile j + 1 is issued between the six MFMAs of tile j (worth 1.5 %: the vector
        // and the matrix instructions of the waves of a SIMD mostly take turns whatever their order -- SQ_VALU_MFMA_COEXEC_CYCLES 0.12 of the kernel's
        // cycles, MFMA-busy 0.38 + vector-busy 0.51 of them -- so what bounds this kernel is the SUM of its 30 MFMAs and ~310 vector instructions per
        // wave and chunk, profiles/r06_stem_wgrad_x6.txt)
        u4 B[2][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) { uint32_t h_, m_, l_; x6_split2(b[0][2 * q], b[0][2 * q + 1], h_, m_, l_); B[0][0][q] = h_; B[0][1][q] = m_; B[0][2][q] = l_; }
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            const int cur = j & 1;
            if (j + 1 < NACC) {
#pragma unroll
                for (int q = 0; q < 4; ++q) { uint32_t h_, m_, l_; x6_split2(b[j + 1][2 * q], b[j + 1][2 * q + 1], h_, m_, l_); B[cur ^ 1][0][q] = h_; B[cur ^ 1][1][q] = m_; B[cur ^ 1][2][q] = l_; }
            }
            x6_mma6(A, B[cur], acc_lo[j], acc_hi[j]);
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // one MFMA ...
                __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);       // ... eight vector instructions in its shadow
            }
        }
    };
    gload(std::integral_constant<int, 0>{});
    if (c_begin + 1 < c_end) gload(std::integral_constant<int, 1>{});
    for (int c = c_begin; c < c_end; c += 3) {
        chunk(std::integral_constant<int, 0>{}, c);
        if (c + 1 < c_end) chunk(std::integral_constant<int, 1>{}, c + 1);
        if (c + 2 < c_end) chunk(std::integral_constant<int, 2>{}, c + 2);
    }
    __syncthreads();                           // every wave is behind its last chunk
    const size_t tap0 = (size_t)((kt_ + p.wk0_t) * p.KH + p.wk0_h) * KW * 4;       // g offset of (kt, kh = 0, kw = 0, cs = 0)
    // the two sub-chunk waves hold partial sums of the SAME outputs: wave wk = 1 hands its sums to wave wk = 0 through LDS, one accumulator
    // per round
    float* image = p.g + (size_t)slice * p.wss;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const f32x16 acc = acc_hi[j] + acc_lo[j];
        if (wk == 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) xch[wm][r][lane] = acc[r];
        }
        __syncthreads();
        if (wk == 0 && gcol[j] >= 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m < p.Cd) {
                    float* dst = image + (size_t)m * p.taps_full * 4 + tap0 + gcol[j];
                    const float v = acc[r] + xch[wm][r][lane];
                    if (p.wss) *dst = v;
                    else atomicAdd(dst, v);
                }
            }
        }
        __syncthreads();
    }
}

// Which kernel family pc_conv_wgrad gives a problem to -- ONE classification for pc_conv_wgrad, pc_conv_wgrad_multi and the host-side
// work accounting (pc_wgrad_work), so the fp32 atomic sum order the goldens were made with cannot drift between copies of the predicates.
enum WgRoute { WG_STEM, WG_ROW3, WG_ROW9, WG_GENERIC };
#ifdef PICONS_DIAG
inline bool wg_ablate() { static const bool a = getenv("PICONS_WGRAD_ABLATE") != nullptr; return a; }
#else
constexpr bool wg_ablate() { return false; }
#endif
inline WgRoute wg_route(const pc_wgrad_desc* d) {
    if (d->Cs == 4 && d->lds % 4 == 0 && d->KW == 7 && d->ntap[2] == 7 && d->wk0[2] == 0 && d->istr[2] == 2 && d->ntap[1] == 7 &&
        d->ntap[0] <= 10 && d->istep[0] == 1 && d->istep[1] == 1 && d->istep[2] == 1 && d->Td == 0 && d->nbatch <= 1 && d->splitk >= 0 &&
        d->Wq % 28 == 0 && !wg_ablate())
        return WG_STEM;
    const bool csb64 = d->Cs % 64 == 0, csb32 = d->Cs % 32 == 0 && d->Cd > 64;
    const int padw = -d->ioff0[2], nprob = d->nbatch > 1 ? d->nbatch : 1;
    const bool row3 = d->KW == 3 && padw == 1 && d->Wq == d->Ws && (csb64 || csb32) && d->Ws % 28 == 0 && nprob == 1 && d->splitk >= 0;
    const bool row9 = d->KW == 9 && padw == 0 && d->Wq == d->Ws - 8 && d->Wq == 20 && csb64 && d->Tq == 1 && d->Hq == 1;   // spectral forms
    if (!wg_ablate() && d->Td == 0 && d->ntap[2] == d->KW && d->wk0[2] == 0 && d->istr[2] == 1 && d->istep[0] == 1 && d->istep[1] == 1 &&
        d->istep[2] == 1 && (row3 || row9))
        return row9 ? WG_ROW9 : WG_ROW3;
    return WG_GENERIC;
}
// Which kernel template instance a problem's launch takes, per route: ONE choice for the launch (wgrad_run), the reporter (pc_wgrad_variant)
// and the accounting (pc_wgrad_work).  Each route has one table; wg_*_inst gives the index, the launch reads .kernel and the reporter .name
// of the same entry.
template <class K> struct WgInst { const char* name; void (*kernel)(K); };
// The stem (WG_STEM problems): the 4th source channel is padding (PC_WG_CS3) -> the 3 real channels of the 7 x 7 taps are packed into five
// accumulators, on the bf16 matrix cores (wgrad4_x6_kernel) when asked for (PC_WG_X6); seven fp32 accumulators otherwise
const WgInst<Wg4K> WG_STEM_INST[] = {{"wgrad4_x6<7,2,7>", wgrad4_x6_kernel<7, 2, 7>},
                                     {"wgrad4<28,7,2,7,pack3>", wgrad4_kernel<28, 7, 2, 7, true>},
                                     {"wgrad4<28,7,2,7>", wgrad4_kernel<28, 7, 2, 7, false>}};
inline int wg_stem_inst(const pc_wgrad_desc* d) {
    if (!(d->flags & PC_WG_CS3)) return 2;
    return (d->flags & PC_WG_X6) ? 0 : 1;
}
inline bool wg_stem_x6(const pc_wgrad_desc* d) { return wg_route(d) == WG_STEM && wg_stem_inst(d) == 0; }
// does the problem's launch multiply on the bf16 matrix cores?  (the 9-tap spectral planes and un-flagged problems stay on fp32 MFMA)
inline bool wg_uses_x6(const pc_wgrad_desc* d) {
    if (!(d->flags & PC_WG_X6)) return false;
    const WgRoute r = wg_route(d);
    return r == WG_ROW3 || r == WG_GENERIC || (r == WG_STEM && wg_stem_x6(d));
}
// 256-column tiles with 16-position chunks for the long-K launches of the generic kernel (128-row and 64-row tiles alike)
inline bool wg_wide(const pc_wgrad_desc* d) {
    if (d->flags & PC_WG_X6) return false;          // the bf16-split kernel keeps 128-column tiles (two accumulators per tile)
    const int64_t P = (int64_t)d->N * d->Tq * d->Hq * d->Wq;
    const int Ntot = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Cs;
    return !wg_ablate() && Ntot >= 512 && P >= 65536;
}
// row-segment kernel geometry (shared by the launch and the accounting)
struct Row3Geo { bool csb64, small_m, x6; int bkp, bm, csb; };
inline Row3Geo wg_row_geo(const pc_wgrad_desc* d, bool row9) {
    Row3Geo r;
    r.csb64 = d->Cs % 64 == 0;
    // 64-row tiles also when they pad at least 20 % less than 128-row tiles (192 = 3 x 64 vs 2 x 128)
    r.small_m = d->Cd <= 64 || row9 || (r.csb64 && cdiv(d->Cd, 64) * 64 * 5 <= cdiv(d->Cd, 128) * 128 * 4);
    r.bkp = row9 ? 20 : ((r.csb64 && r.small_m && d->Ws % 56 == 0) ? 56 : 28);
    r.bm = r.small_m ? 64 : 128;
    r.csb = r.csb64 ? 64 : 32;
    r.x6 = !row9 && (d->flags & PC_WG_X6) != 0;
    if (r.x6) {          // bf16-split kernel: one 32-channel tile of D and of S per wave, whole k16 steps per chunk (the segment's tail reads zeros)
        r.bkp = d->Ws % 56 == 0 ? 64 : 32;
        r.bm = r.csb64 ? 64 : 128;
        r.small_m = r.csb64;
    }
    return r;
}
// the generic kernel's launches for a problem: up to two row ranges [lo, hi) with 64- or 128-row tiles
struct WgSplit { int n; int lo[2], hi[2]; bool small_m[2]; };
inline WgSplit wg_generic_split(const pc_wgrad_desc* d) {
    // 128-row tiles for the bulk.  When the grid is many rounds deep without split-K (PrimaryCaps: 544 = 4*128 + 32
    // rows x 527 column tiles), a remainder of at most 64 channels gets its own launch with 64-row tiles instead
    // of a padded 128-row tile (4.98 vs 5.23 ms); small problems lose more to the second launch than they save
    const int Ntot = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Cs;
    const int full = d->Cd / 128 * 128, rem = d->Cd - full;
    const bool deep = (int64_t)(full / 128) * cdiv(Ntot, 128) * (d->nbatch > 1 ? d->nbatch : 1) >= 1024;
    // 64-row tiles run at ~0.88 of the 128-row tiles' rate: take them when they pad that much less (192 = 3 x 64 vs 2 x 128)
    const double pad128 = (double)cdiv(d->Cd, 128) * 128, pad64 = (double)cdiv(d->Cd, 64) * 64;
    WgSplit w; w.n = 1; w.lo[0] = 0; w.hi[0] = d->Cd; w.small_m[0] = false;
    if (d->Cd <= 64) w.small_m[0] = true;
    else if (rem != 0 && rem <= 64 && deep) { w.n = 2; w.hi[0] = full; w.lo[1] = full; w.hi[1] = d->Cd; w.small_m[1] = true; }
    else if (pad128 > 1.15 * pad64) w.small_m[0] = true;
    return w;
}

const WgInst<Wg3K> WG_ROW_INST[] = {{"wgrad3_x6<64,64,64,2>", wgrad3_x6_kernel<64, 64, 64, 2>},   {"wgrad3_x6<64,32,64,2>", wgrad3_x6_kernel<64, 32, 64, 2>},
                                    {"wgrad3_x6<128,64,32,4>", wgrad3_x6_kernel<128, 64, 32, 4>}, {"wgrad3_x6<128,32,32,4>", wgrad3_x6_kernel<128, 32, 32, 4>},
                                    {"wgrad3<64,20,64,2,9>", wgrad3_kernel<64, 20, 64, 2, 9>},    {"wgrad3<128,28,32,4>", wgrad3_kernel<128, 28, 32, 4>},
                                    {"wgrad3<64,56,64,2>", wgrad3_kernel<64, 56, 64, 2>},         {"wgrad3<64,28,64,2>", wgrad3_kernel<64, 28, 64, 2>},
                                    {"wgrad3<128,28,64,2>", wgrad3_kernel<128, 28, 64, 2>}};
inline int wg_row_inst(const Row3Geo& geo, bool row9) {
    if (geo.x6) return (geo.csb64 && geo.bkp == 64) ? 0 : geo.csb64 ? 1 : geo.bkp == 64 ? 2 : 3;
    if (row9) return 4;
    if (!geo.csb64) return 5;
    if (geo.small_m && geo.bkp == 56) return 6;
    return geo.small_m ? 7 : 8;
}
const WgInst<WgK> WG_GEN_INST[] = {{"wgrad_x6<64,128>", wgrad_x6_kernel<64, 128>},    {"wgrad_x6<128,128>", wgrad_x6_kernel<128, 128>},
                                   {"wgrad<64,256,16>", wgrad_kernel<64, 256, 0, 16>}, {"wgrad<64,128,32>", wgrad_kernel<64, 128>},
                                   {"wgrad<128,256,16>", wgrad_kernel<128, 256, 0, 16>}, {"wgrad<128,128,32>", wgrad_kernel<128, 128>}};
inline int wg_generic_inst(const pc_wgrad_desc* d, bool small_m, bool wide) {
    if (d->flags & PC_WG_X6) return small_m ? 0 : 1;
    if (small_m) return wide ? 2 : 3;
    return wide ? 4 : 5;
}
// what a dry run of wgrad_run reports: K slices (workspace images) of the launch, and its kernel instance(s)
struct WgDry { int nslices; char name[96]; };

}  // namespace

// Host-only work accounting of one pc_conv_wgrad call (no GPU call), see pc_conv_work.  out[5]: multiply-accumulates ISSUED to
// the matrix cores (whole tiles, padded chunks; chunks the row-segment / stem kernels never multiply because their (kt, kh) tap
// reads outside the volume are not counted), EXECUTED on real rows x real columns of the same chunks, VALID (non-padding source
// positions only), the route (0 stem, 1 row-segment 3 taps, 2 row-segment 9 taps, 3 generic split-K) and the number of kernel launches.
extern "C" int pc_wgrad_work(const pc_wgrad_desc* d, int cd_real, int cs_real, double* out) {
    PC_CHECK_ARG(d && out, "pc_wgrad_work: null pointer");
    if (cd_real <= 0) cd_real = d->Cd;
    if (cs_real <= 0) cs_real = d->Cs;
    const int nb = d->nbatch > 1 ? d->nbatch : 1;
    const int Q[3] = {d->Tq, d->Hq, d->Wq}, I[3] = {d->Ts, d->Hs, d->Ws};
    // per dimension and tap: lattice points whose source position exists
    double V[3][16] = {}, Vsum[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        PC_CHECK_ARG(d->ntap[k] >= 1 && d->ntap[k] <= 16, "pc_wgrad_work: ntap out of range");
        for (int a = 0; a < d->ntap[k]; ++a) {
            int cnt = 0;
            for (int q = 0; q < Q[k]; ++q) cnt += (unsigned)(q * d->istr[k] + d->ioff0[k] + a * d->istep[k]) < (unsigned)I[k];
            V[k][a] = cnt; Vsum[k] += cnt;
        }
    }
    const double valid = (double)d->N * nb * Vsum[0] * Vsum[1] * Vsum[2] * cd_real * cs_real;
    const WgRoute route = wg_route(d);
    double issued = 0, executed = 0, launches = 1;
    if (route == WG_STEM) {
        const int inst = wg_stem_inst(d);
        const bool x6 = inst == 0, p3 = inst != 2;
        const int nseg = x6 ? cdiv(d->Wq, 16) : d->Wq / 28, mt = cdiv(d->Cd, 64);
        const double seg = x6 ? 16.0 : 28.0;
        const double nacc = p3 ? (7 * 7 * 3 + 31) / 32 : 7;
        for (int a = 0; a < d->ntap[0]; ++a) {
            const double chunks = (double)d->N * V[0][a] * d->Hq * nseg;          // every kh of the kt tap, all w
            issued += chunks * seg * (mt * 64.0) * nacc * 32.0;
            executed += (double)d->N * V[0][a] * d->Hq * d->Wq * cd_real * (7.0 * 7.0 * cs_real);
        }
    } else if (route == WG_ROW3 || route == WG_ROW9) {
        const Row3Geo r = wg_row_geo(d, route == WG_ROW9);
        const int nseg = cdiv(d->Wq, r.bkp), mt = cdiv(d->Cd, r.bm), ncs = d->Cs / r.csb;
        for (int a = 0; a < d->ntap[0]; ++a)
            for (int b = 0; b < d->ntap[1]; ++b) {
                const double chunks = (double)d->N * nb * V[0][a] * V[1][b] * nseg;
                issued += chunks * r.bkp * (mt * (double)r.bm) * ((double)d->KW * r.csb * ncs);
                executed += chunks * (r.x6 ? (double)d->Wq / nseg : (double)r.bkp) * cd_real * ((double)d->KW * cs_real);       // real positions only
            }
    } else {
        const int64_t P = (int64_t)d->N * d->Tq * d->Hq * d->Wq;
        const int Ntot = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Cs;
        const WgSplit w = wg_generic_split(d);
        launches = w.n;
        for (int i = 0; i < w.n; ++i) {
            const bool wide = wg_wide(d);
            const int bm = w.small_m[i] ? 64 : 128, bn = wide ? 256 : 128, kb = wide ? 16 : BK;
            issued += (double)cdiv(P, kb) * kb * ((double)cdiv(w.hi[i] - w.lo[i], bm) * bm) * ((double)cdiv(Ntot, bn) * bn) * nb;
        }
        executed = (double)P * nb * cd_real * ((double)d->ntap[0] * d->ntap[1] * d->ntap[2] * cs_real);
    }
    out[0] = issued; out[1] = executed; out[2] = valid; out[3] = (double)route; out[4] = launches;
    return PC_OK;
}

namespace {
// floats of one K-slice image of a problem's gradient: g's own layout [Cd][KT*KH*KW][Cs] (x the problems of a batched launch)
inline long long wg_image_floats(const pc_wgrad_desc* d) {
    return d->nbatch > 1 ? (long long)d->gbstride * d->nbatch : (long long)d->Cd * d->KT * d->KH * d->KW * d->Cs;
}

// The K slices of a launch.  wg_deal: `splitk` slices of equal chunk counts; slices that would stay empty are not launched.  wg_slices: the
// same after the clamp every automatic choice takes -- at least 8 chunks per slice, at least one slice.  (The automatic choices fill one round
// of resident-block slots: measured best on the step -- fewer atomics per weight, and the second lane's launches fill what a single round
// leaves idle.  The stem deals its slices per kt tap by its own rule, in wgrad_run.)
struct WgSlices { int chunks_per_split, nsplit; };
inline WgSlices wg_deal(int splitk, int nchunks) {
    const int cps = cdiv(nchunks, splitk);
    return {cps, cdiv(nchunks, cps)};
}
inline WgSlices wg_slices(int want, int nchunks) {
    return wg_deal(std::max(1, std::min(want, nchunks / 8)), nchunks);
}

// The argument checks every weight-gradient entry shares, and the descriptor -> kernel argument copy: one whole-problem launch of atomics
// (mbase / mend / store / wss), which pc_conv_wgrad's generic route then narrows per launch; the tiling (mt, ntl) and the K slices are the
// caller's.  `who` names the entry in the messages, `dma_hint` ends the one message whose advice differs.  Null D / S (a dry run) pass.
int wg_fill(const char* who, const char* dma_hint, const pc_wgrad_desc* d, const float* D, const float* S, float* g, WgK& k) {
    PC_CHECK_ARG(((uintptr_t)D % 16 == 0) && ((uintptr_t)S % 16 == 0), "%s: D/S must be 16-byte aligned", who);
    PC_CHECK_ARG(d->wk0[0] + d->ntap[0] <= d->KT && d->wk0[1] + d->ntap[1] <= d->KH && d->wk0[2] + d->ntap[2] <= d->KW, "%s: trimmed taps exceed the weight extents", who);
    k.D = D; k.S = S; k.g = g;
    k.N = d->N; k.Tq = d->Tq; k.Hq = d->Hq; k.Wq = d->Wq; k.Cd = d->Cd; k.ldd = d->ldd;
    k.Ts = d->Ts; k.Hs = d->Hs; k.Ws = d->Ws; k.Cs = d->Cs; k.lds = d->lds;
    for (int i = 0; i < 3; ++i) { k.istr[i] = d->istr[i]; k.ntap[i] = d->ntap[i]; k.ioff0[i] = d->ioff0[i]; k.istep[i] = d->istep[i]; k.wk0[i] = d->wk0[i]; k.doff[i] = d->doff[i]; }
    k.KH = d->KH; k.KW = d->KW; k.NtotFull = d->KT * d->KH * d->KW * d->Cs;
    k.dlat = d->Td > 0; k.Td = d->Td; k.Hd = d->Hd; k.Wd = d->Wd;
    PC_CHECK_ARG(!k.dlat || (int64_t)d->N * d->Td * d->Hd * d->Wd < (1ll << 31), "%s: D tensor too large", who);
    const int64_t P = (int64_t)d->N * d->Tq * d->Hq * d->Wq;
    PC_CHECK_ARG(P > 0 && P < (1ll << 31) && (int64_t)d->N * d->Ts * d->Hs * d->Ws < (1ll << 31), "%s: position count out of range", who);
    PC_CHECK_ARG((int64_t)d->N * d->Ts * d->Hs * d->Ws * d->lds * 4 < DMA_MAX_BYTES && (k.dlat ? (int64_t)d->N * d->Td * d->Hd * d->Wd : P) * d->ldd * 4 < DMA_MAX_BYTES,
                 "%s: D or S exceeds the 4 GiB the LDS-DMA gather addresses%s", who, dma_hint);
    k.P = (int)P;
    k.Ntot = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Cs;
    k.nchunks = cdiv(P, BK);
    k.mbase = 0; k.mend = d->Cd; k.store = 0; k.wss = 0;
    const bool batched = d->nbatch > 1;
    k.dbs = batched ? d->dbstride : 0; k.sbs = batched ? d->sbstride : 0; k.gbs = batched ? d->gbstride : 0;
    return PC_OK;
}

// weight-gradient launch: carries pc_run_ops_timed's event pair in its own dispatch when one is set (as the conv launches do)
template <class K>
void wg_launch(void (*kernel)(K), dim3 grid, hipStream_t s, const K& arg) {
    if (pc_tl_ev_start) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, s, pc_tl_ev_start, pc_tl_ev_stop, 0, arg);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, arg);
}
}  // namespace

// dry != NULL: no launch -- dry->nslices = the number of K slices (workspace images) the launch would write (pc_wgrad_slices), dry->name = its kernel(s)
static int wgrad_run(const pc_wgrad_desc* d, const float* D, const float* S, float* g, pc_stream s_, WgDry* dry) {
    hipStream_t s = (hipStream_t)s_;
    PC_CHECK_ARG(d && (dry || (D && S && g)), "pc_conv_wgrad: null pointer");
    PC_CHECK_ARG(d->Cd % 4 == 0 && d->Cs % 4 == 0 && d->ldd % 4 == 0 && d->lds % 4 == 0,
                 "pc_conv_wgrad: channel counts / strides must be multiples of 4 (Cd=%d Cs=%d)", d->Cd, d->Cs);
    PC_CHECK_ARG(d->ws_slices >= 0 && !(d->ws_slices > 0 && d->splitk == -1), "pc_conv_wgrad: ws_slices = %d with splitk = %d", d->ws_slices, d->splitk);
    PC_CHECK_ARG(d->nbatch <= 4096, "pc_conv_wgrad: nbatch too large");
    PC_CHECK_ARG(d->splitk != -1 || (d->ntap[0] == d->KT && d->ntap[1] == d->KH && d->ntap[2] == d->KW), "pc_conv_wgrad: splitk = -1 (plain stores) needs every tap present");
    WgK k;
    const int rc = wg_fill("pc_conv_wgrad", ": use a smaller per-GPU batch", d, D, S, g, k);
    if (rc != PC_OK) return rc;
    // ws_slices > 0: g is a workspace of that many K-slice images (wg_image_floats apart); slice k writes image k with plain stores
    const long long wss = d->ws_slices > 0 ? wg_image_floats(d) : 0;
    int nslices = 1;
#ifdef PICONS_DIAG
    static const int abl = getenv("PICONS_WGRAD_ABLATE") ? atoi(getenv("PICONS_WGRAD_ABLATE")) : 0;   // diagnostic build: no tile fetch in the K loop (wrong results)
#endif
    const WgRoute route = wg_route(d);
    if (route == WG_STEM) {
        Wg4K q;
        q.D = D; q.S = S; q.g = g;
        q.N = d->N; q.T = d->Tq; q.H = d->Hq; q.W = d->Wq; q.Cd = d->Cd; q.ldd = d->ldd; q.lds = d->lds;
        q.ntap_t = d->ntap[0]; q.wk0_t = d->wk0[0]; q.wk0_h = d->wk0[1]; q.KH = d->KH;
        q.Ts = d->Ts; q.Hs = d->Hs; q.Wsw = d->Ws; q.istr_t = d->istr[0]; q.istr_h = d->istr[1]; q.ioff_t = d->ioff0[0]; q.ioff_h = d->ioff0[1];
        q.padw = -d->ioff0[2];
        const int inst = wg_stem_inst(d);
        const bool x6 = inst == 0;                      // bf16-split kernel: chunks of two 16-position sub-chunks
        q.nseg = x6 ? cdiv(d->Wq, 16) : d->Wq / 28; q.mt = cdiv(d->Cd, 64); q.taps_full = d->KT * d->KH * d->KW;
        // K slices per kt in proportion to the output t planes whose source plane exists
        int ntv[10], tot = 0;
        for (int a = 0; a < q.ntap_t; ++a) {
            int cnt = 0;
            for (int t = 0; t < d->Tq; ++t) { const int ts = t * q.istr_t + q.ioff_t + a; cnt += ts >= 0 && ts < d->Ts; }
            ntv[a] = cnt; tot += cnt;
        }
        PC_CHECK_ARG(tot > 0, "pc_conv_wgrad: no valid tap");
        // resident-block slots: the fp32 kernel (162 VGPRs, 28 KiB LDS) holds 3 blocks per CU, the bf16-split kernel two
        const int slots = d->splitk > 0 ? d->splitk * q.ntap_t : (x6 ? 512 : 768) / q.mt;
        q.pre[0] = 0;
        for (int a = 0; a < q.ntap_t; ++a) {
            int sl = ntv[a] ? (int)((double)slots * ntv[a] / tot) : 0;
            const int64_t nch = x6 ? ((int64_t)d->N * ntv[a] * d->Hq * q.nseg + 1) / 2 : (int64_t)d->N * ntv[a] * d->Hq * q.nseg;
            if (ntv[a] && sl < 1) sl = 1;
            if (sl > nch / 4 && nch >= 4) sl = (int)(nch / 4);
            if (ntv[a] && sl < 1) sl = 1;
            q.pre[a + 1] = q.pre[a] + sl;
        }
        const dim3 grid((unsigned)(q.pre[q.ntap_t] * q.mt));
        for (int a = 0; a < q.ntap_t; ++a) nslices = std::max(nslices, q.pre[a + 1] - q.pre[a]);
        if (dry) { dry->nslices = nslices; snprintf(dry->name, sizeof dry->name, "%s", WG_STEM_INST[inst].name); return PC_OK; }
        PC_CHECK_ARG(!wss || nslices <= d->ws_slices, "pc_conv_wgrad: the workspace holds %d slice images, this launch writes %d (pc_wgrad_slices)", d->ws_slices, nslices);
        q.wss = wss;
        {   // block order: slices sorted by where in the volume they are (their relative position inside their kt's slice range), kt as tie-break
            const int tot_sl = q.pre[q.ntap_t];
            q.interleave = tot_sl <= 1024;
            if (q.interleave) {
                std::pair<double, int> key[1024];
                for (int a = 0; a < q.ntap_t; ++a) {
                    const int ns = q.pre[a + 1] - q.pre[a];
                    for (int i = 0; i < ns; ++i) key[q.pre[a] + i] = std::make_pair((i + 0.5) / ns, q.pre[a] + i);
                }
                std::sort(key, key + tot_sl);
                for (int i = 0; i < tot_sl; ++i) q.order[i] = (unsigned short)key[i].second;
            }
        }
        wg_launch(WG_STEM_INST[inst].kernel, grid, s, q);
        PC_CHECK_LAUNCH("wgrad4_kernel");
        return PC_OK;
    }
    if (route == WG_ROW3 || route == WG_ROW9) {
        // conv with 3 (padding 1) or 9 (no padding) taps of stride 1 along w and 32- / 64-channel blocks of S: the kw taps share one LDS tile
        const bool row9 = route == WG_ROW9;
        const int padw = -d->ioff0[2], nprob = d->nbatch > 1 ? d->nbatch : 1;
        Wg3K q;
        q.D = D; q.S = S; q.g = g;
        q.N = d->N; q.T = d->Tq; q.H = d->Hq; q.W = d->Wq; q.Cd = d->Cd; q.ldd = d->ldd; q.Cs = d->Cs; q.lds = d->lds;
        q.Ts = d->Ts; q.Hs = d->Hs; q.istr_t = d->istr[0]; q.istr_h = d->istr[1]; q.ioff_t = d->ioff0[0]; q.ioff_h = d->ioff0[1];
        q.ntap_t = d->ntap[0]; q.ntap_h = d->ntap[1]; q.wk0_t = d->wk0[0]; q.wk0_h = d->wk0[1]; q.KH = d->KH;
        q.taps_full = d->KT * d->KH * d->KW;
        q.Wsw = d->Ws; q.padw = padw; q.nprob = nprob; q.dbs = d->dbstride; q.sbs = d->sbstride; q.gbs = d->gbstride;
        const Row3Geo geo = wg_row_geo(d, row9);
        q.nseg = cdiv(d->Wq, geo.bkp);
        q.nchunks = d->N * d->Tq * d->Hq * q.nseg;
        q.mt = cdiv(d->Cd, geo.bm); q.ncs = d->Cs / geo.csb;
        const int64_t tiles = (int64_t)q.mt * q.ncs * q.ntap_t * q.ntap_h;
        // resident-block slots of the variant that will run: the fp32 kernels hold three blocks per CU (two with 56-position segments), the
        // bf16-split ones two -- except wgrad3_x6_kernel<128, 64, 32, 4>, whose 82 KiB of LDS admit ONE block per CU
        const int slots = geo.x6 ? ((!geo.csb64 && geo.bkp == 64) ? 256 : 512) : (geo.bkp == 56 ? 512 : 768);
        const WgSlices sl = wg_slices(d->splitk > 0 ? d->splitk : (d->splitk == -1 ? 1 : (int)((double)slots / (tiles * nprob))), q.nchunks);
        q.chunks_per_split = sl.chunks_per_split; q.nsplit = sl.nsplit;
        q.store = d->splitk == -1;
        const WgInst<Wg3K>& inst = WG_ROW_INST[wg_row_inst(geo, row9)];
        if (dry) { dry->nslices = q.nsplit; snprintf(dry->name, sizeof dry->name, "%s", inst.name); return PC_OK; }
        PC_CHECK_ARG(!wss || q.nsplit <= d->ws_slices, "pc_conv_wgrad: the workspace holds %d slice images, this launch writes %d (pc_wgrad_slices)", d->ws_slices, q.nsplit);
        q.wss = wss;
        wg_launch(inst.kernel, dim3((unsigned)(tiles * q.nsplit * nprob)), s, q);
        PC_CHECK_LAUNCH("wgrad3_kernel");
        return PC_OK;
    }
    bool ws_short = false;
    // one launch of the generic kernel: rows [m_lo, m_hi) of D's channels with 64- or 128-row tiles
    auto launch = [&](int m_lo, int m_hi, bool small_m) {
        // 256-column tiles with 16-position chunks for the long-K launches: 17-25 % less tile traffic per FLOP.  The kernel
        // is bound by the LDS-DMA fill rate, not by the MFMA loop (fetch ablation: 148 TF/s without the fetch, 113-118 with either
        // operand tile alone, 103 with both): 3x3x3 128->128 @112^2 103 -> 115 TF/s, the 64-channel layers 87 -> 92
        const bool wide = wg_wide(d);
        const int bm = small_m ? 64 : 128, bn = wide ? 256 : 128;
        const int nchunks = cdiv(k.P, wide ? 16 : BK);
        const int mt = cdiv(m_hi - m_lo, bm), ntl = cdiv(k.Ntot, bn);
        const int nb = d->nbatch > 1 ? d->nbatch : 1;
        // resident blocks per CU follow the LDS footprint (64 KiB -> 2, 48 KiB -> 3): fill whole rounds of slots and never spill a few
        // blocks into the next (1026 blocks ran ~25 % slower than 1022).  A slice count the caller asks for is taken as it is.
        const int slots = (small_m || wide) ? 768 : 512;
        const WgSlices sl = d->splitk > 0 ? wg_deal(d->splitk, nchunks)
                                          : wg_slices(d->splitk == -1 ? 1 : (int)((double)slots / ((int64_t)mt * ntl * nb)), nchunks);
        WgK kk = k;
        kk.nchunks = nchunks;
        kk.mbase = m_lo; kk.mend = m_hi;
        kk.store = d->splitk == -1;
        kk.chunks_per_split = sl.chunks_per_split; kk.nsplit = sl.nsplit;
        kk.mt = mt; kk.ntl = ntl;
        nslices = std::max(nslices, sl.nsplit);
        const WgInst<WgK>& inst = WG_GEN_INST[wg_generic_inst(d, small_m, wide)];
        if (dry) { const size_t n = strlen(dry->name); snprintf(dry->name + n, sizeof dry->name - n, "%s%s", n ? "+" : "", inst.name); return; }
        if (wss && sl.nsplit > d->ws_slices) { ws_short = true; return; }
        kk.wss = wss;
        const dim3 grid((unsigned)((int64_t)mt * ntl * nb * sl.nsplit));
#ifdef PICONS_DIAG
        // the ablation forms of the 128-column fp32 kernel: 1 no tile fetch in the K loop, 2 + fragment reads hoisted out of the k-step loop,
        // 3 + no barrier per chunk, 4 D tile only, 5 S tile only, 6 position table only
        void (*diag)(WgK) = nullptr;
        if (abl == 2) diag = small_m ? wgrad_kernel<64, 128, 2> : wgrad_kernel<128, 128, 2>;
        else if (abl == 3) diag = small_m ? wgrad_kernel<64, 128, 3> : wgrad_kernel<128, 128, 3>;
        else if (abl == 4) diag = small_m ? wgrad_kernel<64, 128, 4> : wgrad_kernel<128, 128, 4>;
        else if (abl == 5) diag = small_m ? wgrad_kernel<64, 128, 5> : wgrad_kernel<128, 128, 5>;
        else if (abl == 6) diag = small_m ? wgrad_kernel<64, 128, 6> : wgrad_kernel<128, 128, 6>;
        else if (abl) diag = small_m ? wgrad_kernel<64, 128, 1> : wgrad_kernel<128, 128, 1>;
        // tools/wgrad_x6_acc_probe.py: flag bit 4 = one accumulator per tile instead of the hi / lo pair -- 1.1x the fp32 kernel's distance
        // from fp64 where the pair is at 0.5 - 0.6x, at the same speed
        else if ((d->flags & PC_WG_X6) && (d->flags & 4)) diag = small_m ? wgrad_x6_kernel<64, 128, false> : wgrad_x6_kernel<128, 128, false>;
        if (diag) wg_launch(diag, grid, s, kk);
        else
#endif
        wg_launch(inst.kernel, grid, s, kk);
    };
    const WgSplit w = wg_generic_split(d);
    for (int i = 0; i < w.n; ++i) launch(w.lo[i], w.hi[i], w.small_m[i]);
    if (dry) { dry->nslices = nslices; return PC_OK; }
    PC_CHECK_ARG(!ws_short, "pc_conv_wgrad: the workspace holds %d slice images, this launch writes %d (pc_wgrad_slices)", d->ws_slices, nslices);
    PC_CHECK_LAUNCH("wgrad_kernel");
    return PC_OK;
}

extern "C" int pc_conv_wgrad(const pc_wgrad_desc* d, const float* D, const float* S, float* g, pc_stream s) {
    return wgrad_run(d, D, S, g, s, nullptr);
}

extern "C" int pc_wgrad_uses_x6(const pc_wgrad_desc* d) { return d && wg_uses_x6(d) ? 1 : 0; }

extern "C" int pc_wgrad_slices(const pc_wgrad_desc* d) {
    WgDry n = {};
    pc_wgrad_desc e;
    if (!d) { pc_set_error("pc_wgrad_slices: null descriptor"); return -1; }
    e = *d; e.ws_slices = 0;
    return wgrad_run(&e, nullptr, nullptr, nullptr, nullptr, &n) == PC_OK ? n.nslices : -1;
}

// Host-only (no GPU call): the kernel template instance(s) pc_conv_wgrad WOULD launch for this descriptor -- a dry run of the launch code itself.
//   <kernel><template arguments>[+<second launch>]:k<K slices>:<store|atomic|ws>
// wgrad4[_x6] = the 7 x 7 stem, wgrad3[_x6]<BM,BKP,CSB,WMW[,KW]> = row segments, wgrad[_x6]<BM,BN[,positions per chunk]> = generic split-K;
// store = one slice with plain stores (splitk = -1), atomic = fp32 atomics, ws = ordered K-slice images in a workspace (ws_slices > 0)
extern "C" int pc_wgrad_variant(const pc_wgrad_desc* d, char* buf, int cap) {
    PC_CHECK_ARG(d && buf && cap > 0, "pc_wgrad_variant: null pointer");
    WgDry r = {};
    const int rc = wgrad_run(d, nullptr, nullptr, nullptr, nullptr, &r);
    if (rc != PC_OK) return rc;
    PC_CHECK_ARG(d->ws_slices == 0 || r.nslices <= d->ws_slices, "pc_wgrad_variant: the workspace holds %d slice images, this launch writes %d (pc_wgrad_slices)", d->ws_slices, r.nslices);
    const int n = snprintf(buf, (size_t)cap, "%s:k%d:%s", r.name, r.nslices, d->splitk == -1 ? "store" : (d->ws_slices > 0 ? "ws" : "atomic"));
    PC_CHECK_ARG(n > 0 && n < cap, "pc_wgrad_variant: the buffer holds %d bytes", cap);
    return PC_OK;
}


// ---- several weight-gradient problems in one launch ------------------------------------------------------------------------
namespace {

// the problems pc_conv_wgrad would give to the generic split-K kernel (not the stem / row-segment kernels, not a forced split)
bool wg_is_generic(const pc_wgrad_desc* d) {
    if (wg_ablate() || wg_route(d) != WG_GENERIC || d->splitk != 0) return false;
    return !wg_wide(d);          // long-K launches keep their 256-column tiles
}

}  // namespace

extern "C" int pc_conv_wgrad_multi(const pc_wgrad_job* jobs, int njobs, pc_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    PC_CHECK_ARG(jobs && njobs >= 1 && njobs <= 64, "pc_conv_wgrad_multi: jobs=%p njobs=%d (1..64)", (const void*)jobs, njobs);
    std::vector<int> gen;
    for (int j = 0; j < njobs; ++j) {
        if (wg_is_generic(&jobs[j].d)) { gen.push_back(j); continue; }
        const int rc = pc_conv_wgrad(&jobs[j].d, jobs[j].D, jobs[j].S, jobs[j].g, s_);      // stem / row-segment / long-K problems: own launch
        if (rc != PC_OK) return rc;
    }
    for (size_t g0 = 0; g0 < gen.size(); g0 += WG_MAXJOBS) {
        const int n = (int)std::min<size_t>(WG_MAXJOBS, gen.size() - g0);
        if (n == 1) {
            const pc_wgrad_job& q = jobs[gen[g0]];
            const int rc = pc_conv_wgrad(&q.d, q.D, q.S, q.g, s_);
            if (rc != PC_OK) return rc;
            continue;
        }
        WgMulti m;
        m.njobs = n;
        // 64- or 128-row tiles for the whole group: whichever pads less (64-row tiles run at ~0.88 of the 128-row rate)
        double work[2] = {0, 0};
        for (int j = 0; j < n; ++j) {
            const pc_wgrad_desc& d = jobs[gen[g0 + j]].d;
            const double cols = (double)cdiv(d.ntap[0] * d.ntap[1] * d.ntap[2] * d.Cs, 128) * 128, P = (double)d.N * d.Tq * d.Hq * d.Wq * (d.nbatch > 1 ? d.nbatch : 1);
            work[0] += (double)cdiv(d.Cd, 64) * 64 * cols * P;
            work[1] += (double)cdiv(d.Cd, 128) * 128 * cols * P;
        }
        const bool small_m = work[0] < 0.88 * work[1];
        const int bm = small_m ? 64 : 128, slots = small_m ? 768 : 512;
        const double total = work[small_m ? 0 : 1];
        int first = 0;
        for (int j = 0; j < n; ++j) {
            const pc_wgrad_job& q = jobs[gen[g0 + j]];
            WgK& k = m.job[j];
            PC_CHECK_ARG(q.D && q.S && q.g, "pc_conv_wgrad_multi: null pointer");
            PC_CHECK_ARG(q.d.Cd >= 1 && q.d.Cs >= 4 && q.d.Cs % 4 == 0 && q.d.ldd % 4 == 0 && q.d.lds % 4 == 0, "pc_conv_wgrad_multi: channel counts / strides must be multiples of 4");
            PC_CHECK_ARG(q.d.ws_slices == 0, "pc_conv_wgrad_multi: K-slice workspaces are not supported in grouped launches");
            const int rc = wg_fill("pc_conv_wgrad_multi", "", &q.d, q.D, q.S, q.g, k);
            if (rc != PC_OK) return rc;
            const int nb = q.d.nbatch > 1 ? q.d.nbatch : 1;
            k.mt = cdiv(q.d.Cd, bm); k.ntl = cdiv(k.Ntot, 128);
            const int64_t tiles = (int64_t)k.mt * k.ntl * nb;
            // blocks in proportion to the problem's (padded) work: every block of the grid gets about the same number of chunks
            const double w = (double)k.mt * bm * k.ntl * 128 * (double)k.P * nb;
            const WgSlices sl = wg_slices((int)(slots * (w / total) / (double)tiles + 0.5), k.nchunks);
            k.chunks_per_split = sl.chunks_per_split; k.nsplit = sl.nsplit;
            m.first[j] = first;
            first += (int)(tiles * k.nsplit);
        }
        for (int j = n; j <= WG_MAXJOBS; ++j) m.first[j] = first;
        if (small_m) hipLaunchKernelGGL((wgrad_multi_kernel<64, 128>), dim3((unsigned)first), dim3(256), 0, s, m);
        else hipLaunchKernelGGL((wgrad_multi_kernel<128, 128>), dim3((unsigned)first), dim3(256), 0, s, m);
        PC_CHECK_LAUNCH("wgrad_multi_kernel");
    }
    return PC_OK;
}
