// Gather-GEMM convolution family for gfx950: fp32 MFMA (v_mfma_f32_32x32x2_f32), LDS-tiled,
// NDHWC activations, [Co][taps][Ci] weights.  One kernel form covers Conv3d/Conv2d forward
// (TF-SAME padding folded into the gather), conv dgrad, ConvTranspose forward as sub-pixel
// parity classes and ConvTranspose dgrad; the weight gradients are in wgrad.hip.
// Replaces the ATen/cuDNN convolution call sites listed in SURVEY.md §2a (K1, K6, K9-K12).
#include "conv_common.h"
#include <stdlib.h>

namespace {

template <int BM, int BN, int WM, int WN, bool FAST, int ABL = 0>
__global__ __launch_bounds__(256, 2) void conv_gemm_kernel(const ConvK p) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int AR = BM / 32, BR = BN / 32;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1, "4 waves");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [2][BM][LDK]
    float* Bs = smem + 2 * BM * LDK;           // [2][BN][LDK]
    int* rinfo = (int*)(Bs + 2 * BN * LDK);    // [BM][4] n,t0,h0,w0
    int* rout = rinfo + BM * 4;                // [BM] output position index or -1

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = bid % p.ntiles, mtl = bid / p.ntiles;
    const int g = mtl / p.mtiles_g, lt = mtl % p.mtiles_g;
    const int n0 = nt * BN;
    const float* wbase = p.w + (size_t)g * p.wgstride;          // per-group weights (0 stride = shared)
    const float* bbase = p.bias + (size_t)g * p.bgstride;

    for (int r = tid; r < BM; r += 256) {
        const int lm = lt * BM + r;
        int4 info = make_int4(-1, 0, 0, 0);
        int op = -1;
        if (lm < p.Mg) {
            int m = g * p.Mg + lm;
            int n = 0;
            if (p.flags & PC_F_NFAST) { const int ng = p.N / p.groups; n = g * ng + lm % ng; m = lm / ng; }   // sample fastest within the group
            const int wq = m % p.Wq; m /= p.Wq;
            const int hq = m % p.Hq; m /= p.Hq;
            const int tq = m % p.Tq;
            if (!(p.flags & PC_F_NFAST)) n = m / p.Tq;
            info = make_int4(n, tq * p.istr[0] + p.ioff0[0], hq * p.istr[1] + p.ioff0[1],
                             wq * p.istr[2] + p.ioff0[2]);
            op = ((n * p.To + tq * p.ostr[0] + p.ooff[0]) * p.Ho + hq * p.ostr[1] + p.ooff[1]) * p.Wo +
                 wq * p.ostr[2] + p.ooff[2];
        }
        ((int4*)rinfo)[r] = info;
        rout[r] = op;
    }
    __syncthreads();

    const int lrow = tid >> 3, lcol = (tid & 7) * 4;
    int4 ri[AR];
#pragma unroll
    for (int j = 0; j < AR; ++j) ri[j] = ((int4*)rinfo)[lrow + 32 * j];

    f32x4 areg[AR], breg[BR];
    const int tapHW = p.ntap[1] * p.ntap[2];
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    // Branch-free tile fetch: invalid rows / taps read a safe address and are zeroed by a select, so the
    // compiler emits straight-line global_load_dwordx4 instead of one exec-masked branch per load.
    unsigned vmask = 0;   // validity bits of the in-flight tile (A rows then B rows); applied when the tile is stored to LDS
    auto fetch = [&](int dt, int dh, int dw, int wtap, int ci, bool kval) {
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            const int t = ri[j].y + dt, h = ri[j].z + dh, w = ri[j].w + dw;
            const bool v = kval && ri[j].x >= 0 && (unsigned)t < (unsigned)p.Ti &&
                           (unsigned)h < (unsigned)p.Hi && (unsigned)w < (unsigned)p.Wi;
            const size_t pos = (size_t)(((ri[j].x * p.Ti + t) * p.Hi + h) * p.Wi + w);
            const float* src = v ? p.in + pos * p.ldi + ci : p.in;
            areg[j] = *(const f32x4*)src;
            m |= (v ? 1u : 0u) << j;
        }
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            const int co = n0 + lrow + 32 * j;
            const bool v = kval && co < p.Co;
            const float* src = v ? wbase + ((size_t)co * p.wtaps + wtap) * p.ldw + ci : wbase;
            breg[j] = *(const f32x4*)src;
            m |= (v ? 1u : 0u) << (AR + j);
        }
        vmask = m;
    };
    // FAST (Ci % 32 == 0): a K chunk lies inside one tap, so the tap walk is wave-uniform scalar state
    // advanced once per chunk; otherwise decode (tap, ci) per thread with integer division.
    int u_a = 0, u_b = 0, u_c = 0, u_ci = 0;
    auto gload = [&](int c) {
        if (FAST) {
            const int dt = u_a * p.istep[0], dh = u_b * p.istep[1], dw = u_c * p.istep[2];
            const int wtap = ((p.wk0[0] + u_a * p.wkstep[0]) * p.KH + p.wk0[1] + u_b * p.wkstep[1]) * p.KW +
                             p.wk0[2] + u_c * p.wkstep[2];
            fetch(dt, dh, dw, wtap, u_ci + lcol, true);
            u_ci += BK;
            if (u_ci >= p.Ci) {
                u_ci = 0;
                if (++u_c == p.ntap[2]) { u_c = 0; if (++u_b == p.ntap[1]) { u_b = 0; ++u_a; } }
            }
        } else {
            const int kk = c * BK + lcol;
            const bool kval = kk < p.K;
            const int tap = kk / p.Ci, ci = kk - tap * p.Ci;
            const int a_ = tap / tapHW, rem = tap - a_ * tapHW;
            const int b_ = rem / p.ntap[2], c_ = rem - b_ * p.ntap[2];
            const int wtap = ((p.wk0[0] + a_ * p.wkstep[0]) * p.KH + p.wk0[1] + b_ * p.wkstep[1]) * p.KW +
                             p.wk0[2] + c_ * p.wkstep[2];
            fetch(a_ * p.istep[0], b_ * p.istep[1], c_ * p.istep[2], kval ? wtap : 0, kval ? ci : 0, kval);
        }
    };
    auto lstore = [&](int buf) {
        float* a = As + buf * BM * LDK;
        float* b = Bs + buf * BN * LDK;
#pragma unroll
        for (int j = 0; j < AR; ++j) *(f32x4*)(a + (lrow + 32 * j) * LDK + lcol) = ((vmask >> j) & 1u) ? areg[j] : zero4;
#pragma unroll
        for (int j = 0; j < BR; ++j) *(f32x4*)(b + (lrow + 32 * j) * LDK + lcol) = ((vmask >> (AR + j)) & 1u) ? breg[j] : zero4;
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = (p.K + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    const int arow = wm * (BM / WM) + (lane & 31), brow = wn * (BN / WN) + (lane & 31);
    const int kof = (lane >> 5) * 4;
    for (int c = 0; c < nchunks; ++c) {
        const int buf = (ABL >= 1) ? 0 : (c & 1);
        if (ABL == 0 && c + 1 < nchunks) gload(c + 1);
        const float* a = As + buf * BM * LDK + arow * LDK + kof;
        const float* b = Bs + buf * BN * LDK + brow * LDK + kof;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *(const f32x4*)(a + i * 32 * LDK + ((ABL >= 3) ? 0 : ks * 8));
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *(const f32x4*)(b + j * 32 * LDK + ((ABL >= 3) ? 0 : ks * 8));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        if (ABL == 0 && c + 1 < nchunks) lstore(buf ^ 1);
        if (ABL <= 1) __syncthreads();
    }

    // ---- epilogue: C/D map row = (r&3) + 8*(r>>2) + 4*(lane>>5), col = lane&31
    const bool has_bias = p.flags & PC_F_BIAS, has_cs = p.flags & PC_F_CSCALE, accum = p.flags & PC_F_ACCUM;
    if (p.flags & PC_F_BNPART) {
        float* part = p.bnpart + ((size_t)(g * p.mtiles_g + lt) * WM + wm) * 2 * p.Co;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float s = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float v = acc[i][j][r]; s += v; s2 += v * v; }
            s += __shfl_xor(s, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
            if (lane < 32 && col < p.Co) { part[col] = s; part[p.Co + col] = s2; }
        }
    }
    if (ABL == 0 && (p.flags & PC_F_TOUT)) { store_tile_cols<BM, BN, WM, WN, TM, TN>(acc, smem, rout, rinfo, p, n0, wm, wn, lane, tid); return; }
    if (ABL == 0 && store_tile_rows<BM, BN, WM, WN, TM, TN>(acc, smem, rout, rinfo, p, bbase, n0, wm, wn, lane, tid)) return;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int op = rout[row];
            if (op < 0) continue;
            const int nb = rinfo[row * 4];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
                if (col >= p.Co) continue;
                float v = acc[i][j][r];
                if (has_bias) v += bbase[col];
                if (col >= p.act_c0) {
                    if (p.act == PC_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (p.act == PC_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                }
                if (has_cs) v *= p.cscale[(size_t)nb * p.Co + col];
                float* o = p.out + (size_t)op * p.ldo + col;
                if (accum) v += *o;
                *o = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Fast path (Ci % 32 == 0, <= 10 taps per dim): tiles go global -> LDS directly (global_load_lds_dwordx4, no VGPR
// staging, no ds_write), per-row pointers and per-dim tap-validity bit masks are computed once per block, and the
// tap walk is wave-uniform scalar state, so a K chunk costs ~6 VALU per 1 KiB fetched instead of ~20.  The LDS image
// is un-padded [row][32 floats] with the 16-byte slots of a row XOR-swizzled by (row>>1)&7; the swizzle is applied on
// the SOURCE address (LDS-DMA writes lane-linear) and again on the fragment read, which keeps ds_read_b128
// conflict-free for both 16-lane groups.
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

template <int BM, int BN, int WM, int WN, int VAR = 0>
__global__ __launch_bounds__(256, 2) void conv_gemm_glds_kernel(const ConvK p) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int AR = BM / 32, BR = BN / 32;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1, "4 waves");
    // VAR bits 3-4: LDS-DMA ring of 2 + n stages instead of the double buffer.  With one chunk in flight a block waits out the
    // full latency of every tile fetch that misses its XCD's L2 (the activations were just written by a kernel on other XCDs)
    // unless a second resident block covers it -- which the under-filled 28x28 launches (392 blocks on 512 slots) do not have.
    constexpr int ST = 2 + ((VAR >> 3) & 3);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                          // [ST][BM][32]
    float* Bs = smem + ST * BM * BK;           // [ST][BN][32]
    int* rinfo = (int*)(Bs + ST * BN * BK);    // [BM][4] n,t0,h0,w0
    int* rout = rinfo + BM * 4;                // [BM] output position index or -1
    unsigned* tile_or = (unsigned*)(rout + BM);   // OR of every row's tap-validity mask

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    // VAR bit 2 (TAP4): Ci == 4 (the stem: 3 channels padded to one 16-byte piece per tap) - a K chunk is 8 consecutive taps of the
    // tile's tap box instead of 32 channels of one tap, so every 16-byte DMA piece has its own tap (address, validity)
    constexpr bool TAP4 = (VAR & 4) != 0;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int nt = bid % p.ntiles, mtl = bid / p.ntiles;
    const int g = mtl / p.mtiles_g, lt = mtl % p.mtiles_g;
    const int n0 = nt * BN;
    const float* wbase = p.w + (size_t)g * p.wgstride;
    const float* bbase = p.bias + (size_t)g * p.bgstride;
    if (tid == 0) *tile_or = 0u;

    for (int r = tid; r < BM; r += 256) {
        const int lm = lt * BM + r;
        int4 info = make_int4(-1, 0, 0, 0);
        int op = -1;
        if (lm < p.Mg) {
            int m = g * p.Mg + lm;
            int n = 0;
            if (p.flags & PC_F_NFAST) { const int ng = p.N / p.groups; n = g * ng + lm % ng; m = lm / ng; }   // sample fastest within the group
            const int wq = m % p.Wq; m /= p.Wq;
            const int hq = m % p.Hq; m /= p.Hq;
            const int tq = m % p.Tq;
            if (!(p.flags & PC_F_NFAST)) n = m / p.Tq;
            info = make_int4(n, tq * p.istr[0] + p.ioff0[0], hq * p.istr[1] + p.ioff0[1], wq * p.istr[2] + p.ioff0[2]);
            op = ((n * p.To + tq * p.ostr[0] + p.ooff[0]) * p.Ho + hq * p.ostr[1] + p.ooff[1]) * p.Wo + wq * p.ostr[2] + p.ooff[2];
        }
        ((int4*)rinfo)[r] = info;
        rout[r] = op;
    }
    __syncthreads();

    // per-thread fetch rows: row = lrow + 32*j, 16-byte slot (tid&7), source slot XOR-swizzled
    const int lrow = tid >> 3, slot = tid & 7;
    unsigned adma[AR], amask[AR];      // byte offset of the row's tap-origin position from (p.in - abias): never negative
    unsigned bdma[BR];                 // byte offset of the output channel's weight row from wbase, DMA_OOB past Co
    // tap origins may lie in the padding (negative coordinates): the lowest origin position any row can have, as a bias on the base
    const long long apos0 = ((long long)min(p.ioff0[0], 0) * p.Hi + min(p.ioff0[1], 0)) * p.Wi + min(p.ioff0[2], 0);
    const long long abias = -apos0 * p.ldi;      // floats
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        const int row = lrow + 32 * j;
        const int4 ri = ((int4*)rinfo)[row];
        const int ks = TAP4 ? 0 : (slot ^ ((row >> 1) & 7)) * 4;
        unsigned m = 0;
        if (ri.x >= 0) {
            for (int a = 0; a < p.ntap[0]; ++a) m |= ((unsigned)(ri.y + a * p.istep[0]) < (unsigned)p.Ti ? 1u : 0u) << a;
            for (int a = 0; a < p.ntap[1]; ++a) m |= ((unsigned)(ri.z + a * p.istep[1]) < (unsigned)p.Hi ? 1u : 0u) << (10 + a);
            for (int a = 0; a < p.ntap[2]; ++a) m |= ((unsigned)(ri.w + a * p.istep[2]) < (unsigned)p.Wi ? 1u : 0u) << (20 + a);
        }
        amask[j] = m;
        const long long pos = ((long long)(ri.x * p.Ti + ri.y) * p.Hi + ri.z) * p.Wi + ri.w;   // may be "out of range": only used when valid
        adma[j] = (unsigned)(((pos - apos0) * p.ldi + ks) * 4);
    }
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        const int row = lrow + 32 * j, co = n0 + row;
        const int ks = TAP4 ? 0 : (slot ^ ((row >> 1) & 7)) * 4;
        bdma[j] = co < p.Co ? (unsigned)(((size_t)co * p.wtaps * p.ldw + ks) * 4) : DMA_OOB;
    }

    // Tap box of the tile: per dimension a row's valid taps form an interval, and so does their union over the tile.
    // Taps outside the box gather only padding for EVERY row, so the K loop walks the box instead of all taps.
    {
        unsigned mo = 0;
#pragma unroll
        for (int j = 0; j < AR; ++j) mo |= amask[j];
        atomicOr(tile_or, mo);
    }
    __syncthreads();
    const unsigned bo = __builtin_amdgcn_readfirstlane(*tile_or);
    const unsigned bt = bo & 0x3ffu, bh = (bo >> 10) & 0x3ffu, bw = (bo >> 20) & 0x3ffu;
    const bool any_tap = bt && bh && bw;
    const int a_lo = any_tap ? __builtin_ctz(bt) : 0, a_hi = any_tap ? 31 - __builtin_clz(bt) : -1;
    const int b_lo = any_tap ? __builtin_ctz(bh) : 0, b_hi = any_tap ? 31 - __builtin_clz(bh) : -1;
    const int c_lo = any_tap ? __builtin_ctz(bw) : 0, c_hi = any_tap ? 31 - __builtin_clz(bw) : -1;
    int u_a = a_lo, u_b = b_lo, u_c = c_lo, u_ci = 0;
    // TAP4: this thread's logical 16-byte slot of a chunk (the same for all its rows: the swizzle depends on lrow only)
    // is tap (8 * chunk + ksl) of the box in (a, b, c) order
    const int nb_ = b_hi - b_lo + 1, nc_ = c_hi - c_lo + 1;
    int t_a = a_lo, t_b = b_lo, t_c = c_lo;
    if (TAP4 && any_tap) {
        const int ksl = slot ^ ((lrow >> 1) & 7);
        t_c = c_lo + ksl % nc_;
        const int r = ksl / nc_;
        t_b = b_lo + r % nb_; t_a = a_lo + r / nb_;
    }
    auto fetch = [&](int buf) {
        if (TAP4) {
            const bool inb = t_a <= a_hi;
            const long long da = ((long long)(t_a * p.istep[0] * p.Hi + t_b * p.istep[1]) * p.Wi + t_c * p.istep[2]) * p.ldi;
            const unsigned sel = inb ? ((1u << t_a) | (1u << (10 + t_b)) | (1u << (20 + t_c))) : 0xffffffffu;   // never matches out of the box
            const int wtap = ((p.wk0[0] + t_a * p.wkstep[0]) * p.KH + p.wk0[1] + t_b * p.wkstep[1]) * p.KW + p.wk0[2] + t_c * p.wkstep[2];
            const long long db = (long long)wtap * p.ldw;
            float* la = As + buf * BM * BK + (wave * 8) * BK;
            float* lb = Bs + buf * BN * BK + (wave * 8) * BK;
            // every lane has its own tap here: the tap offset is a 32-bit per-lane add (wraps back into range whenever the tap is valid)
            const dma_rsrc_t ra = dma_rsrc(p.in - abias), rb = dma_rsrc(wbase);
            const unsigned dab = (unsigned)(da * 4), dbb = (unsigned)(db * 4);
#pragma unroll
            for (int j = 0; j < AR; ++j) glds16b(ra, ((amask[j] & sel) == sel) ? adma[j] + dab : DMA_OOB, la + j * 32 * BK);
#pragma unroll
            for (int j = 0; j < BR; ++j) glds16b(rb, (bdma[j] != DMA_OOB && inb) ? bdma[j] + dbb : DMA_OOB, lb + j * 32 * BK);
            t_c += 8;
            while (t_c > c_hi) { t_c -= nc_; if (++t_b > b_hi) { t_b = b_lo; ++t_a; } }
            return;
        }
        const long long da = ((long long)(u_a * p.istep[0] * p.Hi + u_b * p.istep[1]) * p.Wi + u_c * p.istep[2]) * p.ldi + u_ci;
        const unsigned sel = (1u << u_a) | (1u << (10 + u_b)) | (1u << (20 + u_c));
        const int wtap = ((p.wk0[0] + u_a * p.wkstep[0]) * p.KH + p.wk0[1] + u_b * p.wkstep[1]) * p.KW + p.wk0[2] + u_c * p.wkstep[2];
        const long long db = (long long)wtap * p.ldw + u_ci;
        float* la = As + buf * BM * BK + (wave * 8) * BK;     // wave-uniform base; the DMA adds lane*16 B itself
        float* lb = Bs + buf * BN * BK + (wave * 8) * BK;
        // the tap / channel-chunk offset is wave-uniform: it moves the resource base (scalar adds), the lane offsets never change
        const dma_rsrc_t ra = dma_rsrc(p.in + (da - abias)), rb = dma_rsrc(wbase + db);
#pragma unroll
        for (int j = 0; j < AR; ++j) glds16b(ra, ((amask[j] & sel) == sel) ? adma[j] : DMA_OOB, la + j * 32 * BK);
#pragma unroll
        for (int j = 0; j < BR; ++j) glds16b(rb, bdma[j], lb + j * 32 * BK);
        u_ci += BK;
        if (u_ci >= p.Ci) {
            u_ci = 0;
            if (++u_c > c_hi) { u_c = c_lo; if (++u_b > b_hi) { u_b = b_lo; ++u_a; } }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nchunks = TAP4 ? ((a_hi - a_lo + 1) * nb_ * nc_ + 7) / 8 : (a_hi - a_lo + 1) * nb_ * nc_ * (p.Ci / BK);
    const int arow = wm * (BM / WM) + (lane & 31), brow = wn * (BN / WN) + (lane & 31);
    const int kh = lane >> 5;
    int aoff[TM], boff[TN], asw[TM], bsw[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) { const int r = arow + i * 32; aoff[i] = r * BK; asw[i] = (r >> 1) & 7; }
#pragma unroll
    for (int j = 0; j < TN; ++j) { const int r = brow + j * 32; boff[j] = r * BK; bsw[j] = (r >> 1) & 7; }
    auto mma_chunk = [&](int buf, int c) {
        const float* a = As + buf * BM * BK;
        const float* b = Bs + buf * BN * BK;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            f32x4 af[TM], bf[TN];
            const int q = ks * 2 + kh;
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *(const f32x4*)(a + aoff[i] + ((q ^ asw[i]) << 2));
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *(const f32x4*)(b + boff[j] + ((q ^ bsw[j]) << 2));
            // TAP4 with PC_F_CI3 (VAR bit 5): a 16-byte slot is one tap's (c0, c1, c2, padding) -- the padding channel's MFMA is not issued
            constexpr int NE = (TAP4 && (VAR & 32)) ? 3 : 4;
#pragma unroll
            for (int e = 0; e < NE; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
            // VAR bit 1 (next tile's DMA issued behind the first MFMA group instead of before the chunk) is set by no instance.
            // The line stays because the surviving instances compile to different instructions without this second call of fetch.
            if (ST == 2 && (VAR & 2) && ks == 0 && c + 1 < nchunks) fetch(buf ^ 1);
        }
    };
    if constexpr (ST == 2) {
        if (nchunks > 0) fetch(0);
        PC_SYNC_DMA();
        for (int c = 0; c < nchunks; ++c) {
            const int buf = c & 1;
            if (!(VAR & 2) && c + 1 < nchunks) fetch(buf ^ 1);
            mma_chunk(buf, c);
            PC_SYNC_DMA();        // the LDS-DMA of chunk c+1 has landed (vmcnt(0), written out: common.h) and the reads of chunk c are fenced
        }
    } else {
        // ring: chunks c .. c+ST-2 in flight while chunk c is multiplied.  Each thread issues AR + BR DMA pieces per chunk, in order,
        // so "chunk c has landed" is vmcnt <= (chunks issued after c) * (AR + BR) for every wave, then the barrier (which also says
        // every wave is done reading the buffer the next fetch overwrites: the one multiplied in the previous iteration).
        constexpr int PIECES = AR + BR;
        for (int c = 0; c < ST - 1 && c < nchunks; ++c) fetch(c);
        int buf = 0, fbuf = (ST - 1) % ST;
        for (int c = 0; c < nchunks; ++c) {
            if (nchunks - 1 - c >= ST - 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((ST - 2) * PIECES) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            if (c + ST - 1 < nchunks) fetch(fbuf);
            mma_chunk(buf, c);
            buf = buf + 1 == ST ? 0 : buf + 1;
            fbuf = fbuf + 1 == ST ? 0 : fbuf + 1;
        }
        __syncthreads();          // the operand ring is reused as the output staging tile
    }

    // ---- epilogue (same as conv_gemm_kernel)
    const bool has_bias = p.flags & PC_F_BIAS, has_cs = p.flags & PC_F_CSCALE, accum = p.flags & PC_F_ACCUM;
    if (p.flags & PC_F_BNPART) {
        float* part = p.bnpart + ((size_t)(g * p.mtiles_g + lt) * WM + wm) * 2 * p.Co;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float s = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float v = acc[i][j][r]; s += v; s2 += v * v; }
            s += __shfl_xor(s, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
            if (lane < 32 && col < p.Co) { part[col] = s; part[p.Co + col] = s2; }
        }
    }
    static_assert(BM * BN <= 2 * (BM + BN) * BK, "output tile fits the operand buffers");
    if (p.flags & PC_F_TOUT) { store_tile_cols<BM, BN, WM, WN, TM, TN>(acc, smem, rout, rinfo, p, n0, wm, wn, lane, tid); return; }
    if (store_tile_rows<BM, BN, WM, WN, TM, TN>(acc, smem, rout, rinfo, p, bbase, n0, wm, wn, lane, tid)) return;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * (BM / WM) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int op = rout[row];
            if (op < 0) continue;
            const int nb = rinfo[row * 4];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * (BN / WN) + j * 32 + (lane & 31);
                if (col >= p.Co) continue;
                float v = acc[i][j][r];
                if (has_bias) v += bbase[col];
                if (col >= p.act_c0) {
                    if (p.act == PC_ACT_RELU) v = fmaxf(v, 0.f);
                    else if (p.act == PC_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
                }
                if (has_cs) v *= p.cscale[(size_t)nb * p.Co + col];
                float* o = p.out + (size_t)op * p.ldo + col;
                if (accum) v += *o;
                *o = v;
            }
        }
    }
}

template <int BM, int BN, int WM, int WN, int VAR>
int launch_conv_glds_v(const ConvK& k, hipStream_t s) {
    constexpr int ST = 2 + ((VAR >> 3) & 3);
    {   // the tiles are fetched with 32-bit lane offsets from a wave-uniform base (glds16b)
        const long long halo = ((long long)(k.ioff0[0] < 0 ? -k.ioff0[0] : 0) * k.Hi + (k.ioff0[1] < 0 ? -k.ioff0[1] : 0)) * k.Wi + (k.ioff0[2] < 0 ? -k.ioff0[2] : 0);
        const long long in_bytes = ((long long)k.N * k.Ti * k.Hi * k.Wi + 2 * halo) * k.ldi * 4, w_bytes = (long long)k.Co * k.wtaps * k.ldw * 4;
        PC_CHECK_ARG(in_bytes < DMA_MAX_BYTES && w_bytes < DMA_MAX_BYTES,
                     "pc_conv_fwd: input (%lld B) or weights (%lld B) exceed the 4 GiB the LDS-DMA gather addresses: use a smaller per-GPU batch", in_bytes, w_bytes);
    }
    const size_t lds = (size_t)(ST * (BM + BN) * BK + BM * 5 + 4) * sizeof(float);
    PC_SET_LDS_ONCE((conv_gemm_glds_kernel<BM, BN, WM, WN, VAR>), lds, "conv_gemm_glds_kernel");
    ConvK p = k;
    p.mtiles_g = cdiv(p.Mg, BM);
    p.ntiles = cdiv(p.Co, BN);
    if (pc_tl_ev_start)
        hipExtLaunchKernelGGL((conv_gemm_glds_kernel<BM, BN, WM, WN, VAR>), dim3(p.groups * p.mtiles_g * p.ntiles), dim3(256), lds, s, pc_tl_ev_start, pc_tl_ev_stop, 0, p);
    else
        hipLaunchKernelGGL((conv_gemm_glds_kernel<BM, BN, WM, WN, VAR>), dim3(p.groups * p.mtiles_g * p.ntiles), dim3(256), lds, s, p);
    PC_CHECK_LAUNCH("conv_gemm_glds_kernel");
    return PC_OK;
}

// Which kernel template instance a launch takes: ONE decision (conv_choice) for the launch (launch_conv) and for the host-only reporter
// (pc_conv_variant), so a test can name the variant it exercises without re-deriving the heuristics.
enum ConvFamily { CF_GLDS, CF_GLDS_TAP8, CF_REG_FAST, CF_REG_RAGGED };
struct ConvChoice { ConvFamily fam; int var; };          // var: VAR of conv_gemm_glds_kernel (ring depth = 2 + ((var >> 3) & 3), bit 5 = PC_F_CI3)

// LDS-DMA ring depth, as VAR of conv_gemm_glds_kernel (8 = 3 stages, 0 = the double buffer): 3 stages for launches of at most one block
// per CU (the 196-block 28x28 layers: 10-25 % faster -- nothing else on the CU covers the latency of a tile fetch that misses L2) where
// two blocks of it still fit a CU, the double buffer otherwise (a ring costs full launches 5-8 %).
inline int conv_glds_var(int bm, int bn, int groups, int Mg, int Co) {
    if (bm * bn <= 128 * 64) {
        const size_t per_stage = (size_t)(bm + bn) * BK * sizeof(float);
        const long long grid = (long long)groups * cdiv(Mg, bm) * cdiv(Co, bn);
        if (grid <= 256 && 3 * per_stage <= 76 * 1024) return 8;
    }
    return 0;
}

// k.in == nullptr (the host-only callers, pc_conv_variant / pc_conv_work, have no pointer) stands for a 16-byte aligned input
inline ConvChoice conv_choice(const ConvK& k, int bm, int bn) {
    const bool fast = k.Ci % BK == 0;
    const bool small_taps = k.ntap[0] <= 10 && k.ntap[1] <= 10 && k.ntap[2] <= 10;
    if (bm == 128 && bn == 64)
        if (k.Ci == 4 && small_taps && ((uintptr_t)k.in % 16 == 0) && k.ldi % 4 == 0 && k.ldw % 4 == 0)
            return {CF_GLDS_TAP8, (k.flags & PC_F_CI3) ? (4 | 32) : 4};
    if (fast && small_taps && ((uintptr_t)k.in % 16 == 0) && k.ldi % 4 == 0) return {CF_GLDS, conv_glds_var(bm, bn, k.groups, k.Mg, k.Co)};
    return {fast ? CF_REG_FAST : CF_REG_RAGGED, 0};
}

template <int BM, int BN, int WM, int WN>
int launch_conv_glds(const ConvK& k, hipStream_t s, int var) {
    if constexpr (BM * BN <= 128 * 64)
        if (var == 8) return launch_conv_glds_v<BM, BN, WM, WN, 8>(k, s);
    return launch_conv_glds_v<BM, BN, WM, WN, 0>(k, s);
}

template <int BM, int BN, int WM, int WN, bool FAST>
int launch_conv2(const ConvK& k, hipStream_t s) {
    const size_t lds = (size_t)(2 * (BM + BN) * LDK + BM * 5) * sizeof(float);
    PC_SET_LDS_ONCE((conv_gemm_kernel<BM, BN, WM, WN, FAST>), lds, "conv_gemm_kernel");
    ConvK p = k;
    p.mtiles_g = cdiv(p.Mg, BM);
    p.ntiles = cdiv(p.Co, BN);
    const int grid = p.groups * p.mtiles_g * p.ntiles;
    if (pc_tl_ev_start) hipExtLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, FAST>), dim3(grid), dim3(256), lds, s, pc_tl_ev_start, pc_tl_ev_stop, 0, p);
    else hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, FAST>), dim3(grid), dim3(256), lds, s, p);
    PC_CHECK_LAUNCH("conv_gemm_kernel");
    return PC_OK;
}

#ifdef PICONS_DIAG
// Diagnostic build only (make diag -> libpicons_diag.so; the product library neither holds these kernels nor reads the variable).
// PICONS_CONV_ABLATE=1|2|3 (tools/ablate_conv.py): 1 = no tile fetch / LDS store in the K loop,
// 2 = also no barrier, 3 = also a fixed fragment address.  Results are WRONG in these modes; they only price phases.
template <int BM, int BN, int WM, int WN, int ABL>
int launch_ablate(const ConvK& k, hipStream_t s) {
    const size_t lds = (size_t)(2 * (BM + BN) * LDK + BM * 5) * sizeof(float);
    (void)hipFuncSetAttribute((const void*)conv_gemm_kernel<BM, BN, WM, WN, true, ABL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    ConvK p = k;
    p.mtiles_g = cdiv(p.Mg, BM);
    p.ntiles = cdiv(p.Co, BN);
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, true, ABL>), dim3(p.groups * p.mtiles_g * p.ntiles), dim3(256), lds, s, p);
    PC_CHECK_LAUNCH("conv_gemm_kernel(ablate)");
    return PC_OK;
}
#endif

template <int BM, int BN, int WM, int WN>
int launch_conv(const ConvK& k, hipStream_t s) {
#ifdef PICONS_DIAG
    static const int abl = getenv("PICONS_CONV_ABLATE") ? atoi(getenv("PICONS_CONV_ABLATE")) : 0;
    if (abl && k.Ci % BK == 0 && BM == 128 && BN >= 64) {
        if (abl == 1) return launch_ablate<BM, BN, WM, WN, 1>(k, s);
        if (abl == 2) return launch_ablate<BM, BN, WM, WN, 2>(k, s);
        return launch_ablate<BM, BN, WM, WN, 3>(k, s);
    }
#endif
    const ConvChoice c = conv_choice(k, BM, BN);
    if constexpr (BM == 128 && BN == 64)
        if (c.fam == CF_GLDS_TAP8)
            return (c.var & 32) ? launch_conv_glds_v<BM, BN, WM, WN, 4 | 32>(k, s) : launch_conv_glds_v<BM, BN, WM, WN, 4>(k, s);
    if (c.fam == CF_GLDS) return launch_conv_glds<BM, BN, WM, WN>(k, s, c.var);
    return c.fam == CF_REG_FAST ? launch_conv2<BM, BN, WM, WN, true>(k, s) : launch_conv2<BM, BN, WM, WN, false>(k, s);
}

// tile choice: minimise padded work, prefer larger tiles when the grid still fills the chip
struct TileCfg { int bm, bn, wm; };
inline TileCfg choose_tile(int Mg, int groups, int Co, int Ci) {
    if (Ci == 4) return {128, 64, 2};          // one 16-byte piece per tap: the 8-taps-per-chunk LDS-DMA variant has this tile only
    const TileCfg cand[] = {{128, 128, 2}, {128, 64, 2}, {64, 64, 2}, {128, 32, 4}};
    double best = 1e30; TileCfg bc = cand[0];
    for (const TileCfg& c : cand) {
        const double mt = (double)groups * cdiv(Mg, c.bm), ntl = cdiv(Co, c.bn);
        const double blocks = mt * ntl;
        const double work = blocks * c.bm * c.bn;                 // padded MACs per unit K
        const double eff = (c.bm * c.bn) / (double)(c.bm + c.bn); // operand reuse
        // waves of blocks over 512 slots (2 blocks/CU); partial last wave costs a full one
        const double slots = 512.0, wavesq = ceil(blocks / slots);
        const double fill = blocks / (wavesq * slots);
        const double cost = work / (fill > 0.9 ? 1.0 : fill / 0.9) * (1.0 + 8.0 / eff);   // swept 0.35..1.0 on the step
        if (cost < best) { best = cost; bc = c; }
    }
    return bc;
}

// The tile pc_conv_fwd launches for a descriptor (shared with the host-side work accounting, pc_conv_work).
inline TileCfg launch_tile(const pc_conv_desc* d, int groups) {
    const int64_t Mg = (int64_t)(d->N / groups) * d->Tq * d->Hq * d->Wq;
    TileCfg c = choose_tile((int)Mg, groups, d->Co, d->Ci);
    if (d->flags & PC_F_NFAST) {
        // n-fastest rows: a tile should hold whole groups of N samples of consecutive w so its tap box is tight;
        // when Wq*N is not a multiple of 128 use 64-row tiles (28 w x 16 samples = 7 tiles of 64, none straddles a row)
        const long long per_row = (long long)d->Wq * (d->N / groups);
        if (per_row % 128 != 0 && per_row % 64 == 0) { c.bm = 64; c.bn = d->Co >= 128 ? 128 : 64; c.wm = d->Co >= 128 ? 1 : 2; }
    }
    return c;
}

// The template instance <BM, BN, WM, WN> pc_conv_fwd instantiates for launch_tile's answer (anything else runs on the 128 x 32 tile)
struct ConvInst { int bm, bn, wm, wn; };
inline ConvInst conv_inst(const pc_conv_desc* d, int groups) {
    const TileCfg c = launch_tile(d, groups);
    if (c.bm == 64 && c.bn == 128) return {64, 128, 1, 4};
    if (c.bm == 128 && c.bn == 128) return {128, 128, 2, 2};
    if (c.bm == 128 && c.bn == 64) return {128, 64, 2, 2};
    if (c.bm == 64 && c.bn == 64) return {64, 64, 2, 2};
    return {128, 32, 4, 1};
}

// conv_choice's answer for a descriptor alone (the host-only reporters: no operand pointers, so an aligned input is assumed)
inline ConvChoice conv_choice_desc(const pc_conv_desc* d, int groups, int bm, int bn) {
    ConvK k = {};
    k.Ci = d->Ci; k.ldi = d->ldi; k.ldw = d->ldw; k.Co = d->Co; k.flags = d->flags; k.groups = groups;
    k.Mg = (int)((int64_t)(d->N / groups) * d->Tq * d->Hq * d->Wq);
    for (int i = 0; i < 3; ++i) k.ntap[i] = d->ntap[i];
    return conv_choice(k, bm, bn);
}

}  // namespace

// Host-only accounting of the multiply-accumulates one pc_conv_fwd launch performs (no GPU call).  It walks the launch's tiles
// with the kernel's own row order (conv_gemm_glds_kernel: rinfo / amask / tap box) and counts, per tile, the K the block's loop
// really walks.  out[0] = MACs ISSUED to the matrix cores (whole BM x BN tiles, what an MFMA instruction counter sees),
// out[1] = MACs EXECUTED on real outputs (real rows x real columns x the tile's K: padding taps INSIDE the tap box included),
// out[2] = VALID MACs (taps that read inside the volume only, real channels), out[3] = blocks, out[4] = BM, out[5] = BN,
// out[6] = 1 if the LDS-DMA kernel (tap box) runs, 0 for the register-staged kernel (flattened K, no tap skipping).
// ci_real / co_real: channels that are not padding (0 = Ci / Co).
extern "C" int pc_conv_work(const pc_conv_desc* d, int ci_real, int co_real, double* out) {
    PC_CHECK_ARG(d && out, "pc_conv_work: null pointer");
    const int groups = d->groups > 0 ? d->groups : 1;
    PC_CHECK_ARG(d->N % groups == 0, "pc_conv_work: N %% groups");
    const int64_t Mg = (int64_t)(d->N / groups) * d->Tq * d->Hq * d->Wq;
    TileCfg c = launch_tile(d, groups);
    const bool x6 = pc_x6_eligible(d);                   // PC_F_X6: the bf16-split kernel's tiles (conv_x6.hip), always with the tap box
    if (x6) { const X6Tile t = pc_x6_tile(d, groups); c.bm = t.bm; c.bn = t.bn; c.wm = t.wm; }
    if (ci_real <= 0) ci_real = d->Ci;
    if (co_real <= 0) co_real = d->Co;
    // the kernel family is the launch's own decision; the accounting has no input pointer, which conv_choice takes for an aligned one
    const ConvFamily fam = x6 ? CF_GLDS : conv_choice_desc(d, groups, c.bm, c.bn).fam;
    const bool tap4 = fam == CF_GLDS_TAP8;
    const bool glds = fam == CF_GLDS || tap4;
    const int64_t mtiles = cdiv(Mg, c.bm), ntiles = cdiv(d->Co, c.bn);
    const int ng = d->N / groups;
    const int I[3] = {d->Ti, d->Hi, d->Wi};
    double issued = 0, executed = 0, valid = 0;
    const int Kflat = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Ci;
    for (int g = 0; g < groups; ++g)
        for (int64_t lt = 0; lt < mtiles; ++lt) {
            unsigned box[3] = {0, 0, 0};
            int64_t rows = 0;
            double vtaps = 0;
            for (int r = 0; r < c.bm; ++r) {
                const int64_t lm = lt * c.bm + r;
                if (lm >= Mg) break;
                ++rows;
                int64_t m = (int64_t)g * Mg + lm;
                if (d->flags & PC_F_NFAST) m = lm / ng;
                const int q[3] = {(int)((m / ((int64_t)d->Wq * d->Hq)) % d->Tq), (int)((m / d->Wq) % d->Hq), (int)(m % d->Wq)};
                int nv[3];
                for (int k = 0; k < 3; ++k) {
                    nv[k] = 0;
                    const int base = q[k] * d->istr[k] + d->ioff0[k];
                    for (int a = 0; a < d->ntap[k]; ++a)
                        if ((unsigned)(base + a * d->istep[k]) < (unsigned)I[k]) { box[k] |= 1u << a; ++nv[k]; }
                }
                vtaps += (double)nv[0] * nv[1] * nv[2];
            }
            double Ktile, Kreal;                     // K the block walks (kernel channels) / the same in real channels
            if (glds) {
                int ext[3];
                bool any = box[0] && box[1] && box[2];
                for (int k = 0; k < 3; ++k) ext[k] = any ? (32 - __builtin_clz(box[k])) - __builtin_ctz(box[k]) : 0;
                const double taps = (double)ext[0] * ext[1] * ext[2];
                if (tap4) {                          // 8 taps per chunk; with PC_F_CI3 three MFMAs per 16-byte piece instead of four
                    const double ch = (d->flags & PC_F_CI3) ? 3.0 : 4.0;
                    Ktile = ceil(taps / 8.0) * 8.0 * ch;
                    Kreal = taps * ci_real;
                } else {
                    Ktile = taps * d->Ci;
                    Kreal = taps * ci_real;
                }
            } else {
                Ktile = (double)cdiv(Kflat, BK) * BK;
                Kreal = (double)d->ntap[0] * d->ntap[1] * d->ntap[2] * ci_real;
            }
            // the bf16-split kernel: a wave owns 32 rows of the tile and multiplies nothing when none of them is a real row
            issued += (double)(x6 ? cdiv(rows, 32) * 32 : c.bm) * c.bn * ntiles * Ktile;
            executed += (double)rows * co_real * Kreal;
            valid += vtaps * ci_real * co_real;
        }
    out[0] = issued; out[1] = executed; out[2] = valid; out[3] = (double)groups * mtiles * ntiles; out[4] = c.bm; out[5] = c.bn; out[6] = glds ? 1.0 : 0.0;
    return PC_OK;
}

extern "C" int pc_conv_bnpart_rows(const pc_conv_desc* d) {
    const int groups = d->groups > 0 ? d->groups : 1;
    const int64_t Mg = (int64_t)(d->N / groups) * d->Tq * d->Hq * d->Wq;
    if (pc_x6_eligible(d)) { const X6Tile t = pc_x6_tile(d, groups); return groups * cdiv(Mg, t.bm) * t.wm; }
    const TileCfg c = choose_tile((int)Mg, groups, d->Co, d->Ci);
    return groups * cdiv(Mg, c.bm) * c.wm;
}

static int pc_conv_fwd_g(const pc_conv_desc* d, int groups, const float* in, const float* w, const float* bias,
                  const float* cscale, float* out, float* bnpart, hipStream_t s) {
    PC_CHECK_ARG(d && in && w && out, "pc_conv_fwd: null pointer");
    PC_CHECK_ARG(!(d->flags & PC_F_X6), "pc_conv_fwd: PC_F_X6 descriptors go to pc_conv_fwd_x6 (weight planes)");
    PC_CHECK_ARG(d->Ci % 4 == 0 && d->ldi % 4 == 0 && d->ldw % 4 == 0, "pc_conv_fwd: Ci/ldi/ldw must be multiples of 4 (Ci=%d ldi=%d ldw=%d)", d->Ci, d->ldi, d->ldw);
    PC_CHECK_ARG(groups >= 1 && d->N % groups == 0, "pc_conv_fwd: N %% groups");
    PC_CHECK_ARG(!(d->flags & PC_F_BIAS) || bias, "pc_conv_fwd: bias flag without pointer");
    PC_CHECK_ARG(!(d->flags & PC_F_CSCALE) || cscale, "pc_conv_fwd: cscale flag without pointer");
    PC_CHECK_ARG(!(d->flags & PC_F_BNPART) || bnpart, "pc_conv_fwd: bnpart flag without pointer");
    PC_CHECK_ARG(!(d->flags & PC_F_NFAST) || !(d->flags & (PC_F_BNPART | PC_F_CSCALE)), "pc_conv_fwd: NFAST cannot be combined with BN partials / cscale");
    PC_CHECK_ARG(!(d->flags & PC_F_TOUT) || (!(d->flags & (PC_F_BNPART | PC_F_CSCALE | PC_F_BIAS | PC_F_ACCUM | PC_F_NFAST)) && d->act == PC_ACT_NONE),
                 "pc_conv_fwd: channel-major output (PC_F_TOUT) is for plain launches only");
    PC_CHECK_ARG(((uintptr_t)in % 16 == 0) && ((uintptr_t)w % 16 == 0), "pc_conv_fwd: in/w must be 16-byte aligned");
    ConvK k;
    k.in = in; k.w = w; k.bias = bias; k.cscale = cscale; k.out = out; k.bnpart = bnpart;
    k.N = d->N; k.Ti = d->Ti; k.Hi = d->Hi; k.Wi = d->Wi; k.Ci = d->Ci; k.ldi = d->ldi;
    k.Tq = d->Tq; k.Hq = d->Hq; k.Wq = d->Wq; k.To = d->To; k.Ho = d->Ho; k.Wo = d->Wo; k.Co = d->Co; k.ldo = d->ldo;
    for (int i = 0; i < 3; ++i) {
        k.ostr[i] = d->ostr[i]; k.ooff[i] = d->ooff[i]; k.istr[i] = d->istr[i]; k.ntap[i] = d->ntap[i];
        k.ioff0[i] = d->ioff0[i]; k.istep[i] = d->istep[i]; k.wk0[i] = d->wk0[i]; k.wkstep[i] = d->wkstep[i];
        PC_CHECK_ARG(d->ntap[i] >= 1, "pc_conv_fwd: ntap < 1");
    }
    k.KH = d->KH; k.KW = d->KW; k.wtaps = d->KT * d->KH * d->KW; k.ldw = d->ldw;
    k.K = d->ntap[0] * d->ntap[1] * d->ntap[2] * d->Ci;
    const int64_t M = (int64_t)d->N * d->Tq * d->Hq * d->Wq;
    PC_CHECK_ARG(M > 0 && M < (1ll << 31) && (int64_t)d->N * d->To * d->Ho * d->Wo < (1ll << 31) && (int64_t)d->N * d->Ti * d->Hi * d->Wi < (1ll << 31), "pc_conv_fwd: position count out of range");
    k.M = (int)M; k.groups = groups; k.Mg = (int)(M / groups);
    k.act = d->act; k.flags = d->flags & ~F_SCALAR_EPI; k.act_c0 = d->act_c0; k.wgstride = d->wgstride; k.bgstride = d->bgstride;
    const ConvInst c = conv_inst(d, groups);
    if (c.bm == 64 && c.bn == 128) return launch_conv<64, 128, 1, 4>(k, s);
    if (c.bm == 128 && c.bn == 128) return launch_conv<128, 128, 2, 2>(k, s);
    if (c.bm == 128 && c.bn == 64) return launch_conv<128, 64, 2, 2>(k, s);
    if (c.bm == 64 && c.bn == 64) return launch_conv<64, 64, 2, 2>(k, s);
    return launch_conv<128, 32, 4, 1>(k, s);
}

extern "C" int pc_conv_fwd(const pc_conv_desc* d, const float* in, const float* w, const float* bias,
                           const float* cscale, float* out, float* bnpart, pc_stream s) {
    return pc_conv_fwd_g(d, d && d->groups > 0 ? d->groups : 1, in, w, bias, cscale, out, bnpart, (hipStream_t)s);
}

// Host-only (no GPU call): the kernel template instance pc_conv_fwd -- or, for a PC_F_X6 descriptor, pc_conv_fwd_x6_ws with a workspace of
// ws_floats floats -- WOULD launch for this descriptor with 16-byte aligned operands, from the decision code the launches themselves run
// (conv_inst / conv_choice here, pc_x6_tile / x6_split in conv_x6.hip).  One string:
//   conv:<glds|glds_tap8|reg_fast|reg_ragged>:<BM>x<BN>:w<WM>x<WN>[:st<ring depth>][:ci3]      (glds = LDS-DMA, reg = register-staged gather)
//   x6:<BM>x<BN>:w<WM>x<WN>:ks<K slices of the tail tiles, 1 = no tail split>[:mfast]        (mfast = row tiles fastest in the block order)
extern "C" int pc_conv_variant(const pc_conv_desc* d, int64_t ws_floats, char* buf, int cap) {
    PC_CHECK_ARG(d && buf && cap > 0, "pc_conv_variant: null pointer");
    const int groups = d->groups > 0 ? d->groups : 1;
    PC_CHECK_ARG(d->N > 0 && d->N % groups == 0, "pc_conv_variant: N %% groups");
    if (d->flags & PC_F_X6) return pc_x6_variant(d, ws_floats, buf, cap);
    PC_CHECK_ARG(d->Ci % 4 == 0 && d->ldi % 4 == 0 && d->ldw % 4 == 0, "pc_conv_variant: Ci/ldi/ldw must be multiples of 4 (Ci=%d ldi=%d ldw=%d)", d->Ci, d->ldi, d->ldw);
    const ConvInst t = conv_inst(d, groups);
    const ConvChoice c = conv_choice_desc(d, groups, t.bm, t.bn);
    static const char* const fam[] = {"glds", "glds_tap8", "reg_fast", "reg_ragged"};
    int n = snprintf(buf, (size_t)cap, "conv:%s:%dx%d:w%dx%d", fam[c.fam], t.bm, t.bn, t.wm, t.wn);
    if (n > 0 && n < cap && (c.fam == CF_GLDS || c.fam == CF_GLDS_TAP8)) n += snprintf(buf + n, (size_t)(cap - n), ":st%d%s", 2 + ((c.var >> 3) & 3), (c.var & 32) ? ":ci3" : "");
    PC_CHECK_ARG(n > 0 && n < cap, "pc_conv_variant: the buffer holds %d bytes", cap);
    return PC_OK;
}
