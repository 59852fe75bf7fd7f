// HBM-bound members of the train step for gfx950: BatchNorm3d(train)+ReLU fwd/bwd with
// two-pass batch groups, MaxPool3d SAME fwd/bwd, Dropout3d channel scale, activation/bias
// backward, layout changes, batched transposes for weight re-layout, fill/axpy, fused Adam.
// All loads/stores are float4 along the channel (innermost NDHWC) dimension.
#include "common.h"
#include <stdlib.h>

namespace {

// ------------------------------------------------------------------------------ BN forward
// part [groups][npg][2][C]; stat [groups][4][C] = mean, invstd, scale, shift.
constexpr int FIN_RL = 16;   // row lanes of the partial-sum finalize kernels
constexpr int FIN_CL = 16;   // channels per block: C / 16 blocks, so that even the 64-channel layers spread over a few CUs
constexpr int FIN_T = FIN_RL * FIN_CL;
// 256-thread blocks (one wave per SIMD, <= 32 registers, 4 KB of LDS): these kernels are a handful of blocks on the step's dependency chain, and
// they run beside GEMM launches that fill every resident-block slot for hundreds of microseconds.  As 1024-thread blocks (four waves per SIMD and
// 128 registers per lane at once on ONE CU) they waited for a CU to drain: 35 us on average in the four-lane step, up to 290, against 5 alone.

// sum over partial rows [npg][2][C] for FIN_CL channels; result valid on threads with rl == 0
template <typename TP>
__device__ __forceinline__ void partial_colsum(const TP* __restrict__ part, int npg, int C, int c, int rl,
                                               double (*sh)[FIN_RL][FIN_CL], int cl, double& s, double& s2) {
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (c < C) {
        int i = rl;
        for (; i + 3 * FIN_RL < npg; i += 4 * FIN_RL) {          // four independent rows in flight per thread
            TP x[4], y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { const TP* q = part + (size_t)(i + u * FIN_RL) * 2 * C + c; x[u] = q[0]; y[u] = q[C]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] += (double)x[u]; b[u] += (double)y[u]; }
        }
        for (; i < npg; i += FIN_RL) { const TP* q = part + (size_t)i * 2 * C + c; a[0] += (double)q[0]; b[0] += (double)q[C]; }
    }
    sh[0][rl][cl] = (a[0] + a[1]) + (a[2] + a[3]); sh[1][rl][cl] = (b[0] + b[1]) + (b[2] + b[3]);
    __syncthreads();
    s = 0; s2 = 0;
    if (rl == 0)
        for (int r = 0; r < FIN_RL; ++r) { s += sh[0][r][cl]; s2 += sh[1][r][cl]; }
    __syncthreads();
}

// Two-stage form for layers with thousands of partial rows (the stem leaves 2 x 6272 per batch group: one block per 16 channels walked
// them in 85 us, alone on the dependency chain at the very start of a step): stage 1 spreads the rows of a group over FIN_S blocks per
// channel block and leaves FIN_S double-precision partial rows, stage 2 is the finalize kernel over those.  Fixed order: deterministic.
constexpr int FIN_S = 32;
__global__ __launch_bounds__(FIN_T) void bn_partial_reduce_kernel(const float* __restrict__ part, int npg, int C, double* __restrict__ ws) {
    __shared__ double sh[2][FIN_RL][FIN_CL];
    const int cl = threadIdx.x % FIN_CL, rl = threadIdx.x / FIN_CL;
    const int c = blockIdx.x * FIN_CL + cl, sl = blockIdx.y, g = blockIdx.z;
    const int per = (npg + FIN_S - 1) / FIN_S, r0 = sl * per, r1 = min(npg, r0 + per);
    double s, s2;
    partial_colsum(part + ((size_t)g * npg + r0) * 2 * C, max(0, r1 - r0), C, c, rl, sh, cl, s, s2);
    if (rl == 0 && c < C) {
        double* o = ws + ((size_t)g * FIN_S + sl) * 2 * C;
        o[c] = s; o[C + c] = s2;
    }
}

template <typename TP>
__global__ __launch_bounds__(FIN_T) void bn_finalize_kernel(const TP* __restrict__ part, int npg, int groups,
                                                           int C, double count, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float mom,
                                                           float* rmean, float* rvar, float* __restrict__ stat) {
    __shared__ double sh[2][FIN_RL][FIN_CL];
    const int cl = threadIdx.x % FIN_CL, rl = threadIdx.x / FIN_CL;
    const int c = blockIdx.x * FIN_CL + cl;
    float rm = 0.f, rv = 0.f;
    const bool upd = (rmean != nullptr) && c < C && rl == 0;
    if (upd) { rm = rmean[c]; rv = rvar[c]; }
    for (int g = 0; g < groups; ++g) {
        double s, s2;
        partial_colsum(part + (size_t)g * npg * 2 * C, npg, C, c, rl, sh, cl, s, s2);
        if (rl == 0 && c < C) {
            const double mean = s / count;
            double var = s2 / count - mean * mean;
            if (var < 0.0) var = 0.0;
            const float invstd = (float)(1.0 / sqrt(var + (double)eps));
            const float sc = gamma[c] * invstd;
            float* st = stat + (size_t)g * 4 * C;
            st[c] = (float)mean; st[C + c] = invstd; st[2 * C + c] = sc; st[3 * C + c] = beta[c] - (float)mean * sc;
            if (upd) {
                const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
                rm = (1.f - mom) * rm + mom * (float)mean;
                rv = (1.f - mom) * rv + mom * (float)unb;
            }
        }
    }
    if (upd) { rmean[c] = rm; rvar[c] = rv; }
}

__global__ __launch_bounds__(256) void bn_eval_stat_kernel(const float* gamma, const float* beta, const float* rm,
                                                           const float* rv, float eps, int C, float* stat) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float invstd = 1.0f / sqrtf(rv[c] + eps), sc = gamma[c] * invstd;
    stat[c] = rm[c]; stat[C + c] = invstd; stat[2 * C + c] = sc; stat[3 * C + c] = beta[c] - rm[c] * sc;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ stat,
                                                       int C4, int64_t total4, int64_t rows_per_group, float* __restrict__ y,
                                                       int ldy, int relu) {
    const int C = C4 * 4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
        const unsigned row = (unsigned)idx / (unsigned)C4;          // total4 < 2^31 (checked by the caller): 32-bit index math
        const int c = (int)((unsigned)idx - row * C4) * 4;
        const float* st = stat + (size_t)(row / (unsigned)rows_per_group) * 4 * C;
        const f32x4 v = *(const f32x4*)(z + (size_t)row * ldz + c);
        const f32x4 sc = *(const f32x4*)(st + 2 * C + c), sh = *(const f32x4*)(st + 3 * C + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t = v[e] * sc[e] + sh[e]; o[e] = relu ? fmaxf(t, 0.f) : t; }
        *(f32x4*)(y + (size_t)row * ldy + c) = o;
    }
}

// ------------------------------------------------------------------------------ column reductions
// Per-channel reduction of two quantities over a block of rows for the BatchNorm backward (sum dzh, sum dzh*xhat).
struct RedP {
    const float* a; int lda; const float* b; int ldb; const float* stat; int C4; int64_t rows, rows_per_group;
    int64_t rows_per_block; int act; float* part;   // part [nblk][2][C]
    int64_t a_gs, b_gs, stat_gs, part_gs;           // blockIdx.y = batch group: element strides of a, b, stat, part (0 for one group)
};

__global__ __launch_bounds__(256) void colreduce_kernel(RedP p) {
    p.a += blockIdx.y * p.a_gs; p.b += blockIdx.y * p.b_gs; p.stat += blockIdx.y * p.stat_gs; p.part += blockIdx.y * p.part_gs;
    const int C4 = p.C4, C = C4 * 4;
    const int rpi = 256 / C4;                       // rows per iteration
    const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4;
    const bool active = rl < rpi;
    const int64_t r0 = (int64_t)blockIdx.x * p.rows_per_block;
    const int64_t r1 = min(p.rows, r0 + p.rows_per_block);
    // A thread's sum runs over thousands of rows of mixed sign (a BatchNorm bias gradient is ~1e-3 of sum |dy|): fp32 chains of that
    // length left the BN parameter gradients 3x further from an fp64 run than the fp32 reference's (pairwise) sums.  Short fp32 runs of
    // four rows, flushed into double: the kernel stays HBM-bound.
    double sd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (active) {
        const int c = c4 * 4;
        float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int run = 0;
        for (int64_t r = r0 + rl; r < r1; r += rpi) {
            const f32x4 dy = *(const f32x4*)(p.a + r * p.lda + c);
            const f32x4 zz = *(const f32x4*)(p.b + r * p.ldb + c);
            const float* st = p.stat;                  // one batch group per blockIdx.y (p.rows == p.rows_per_group)
            const f32x4 mean = *(const f32x4*)(st + c), inv = *(const f32x4*)(st + C + c);
            const f32x4 sc = *(const f32x4*)(st + 2 * C + c), sh_ = *(const f32x4*)(st + 3 * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float yv = zz[e] * sc[e] + sh_[e];
                const float d = (p.act == PC_ACT_RELU && !(yv > 0.f)) ? 0.f : dy[e];
                s[e] += d;
                s[4 + e] += d * (zz[e] - mean[e]) * inv[e];
            }
            if (++run == 4) {
                run = 0;
#pragma unroll
                for (int e = 0; e < 8; ++e) { sd[e] += (double)s[e]; s[e] = 0.f; }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) sd[e] += (double)s[e];
    }
    __shared__ double shd[256 * 8];
#pragma unroll
    for (int e = 0; e < 8; ++e) shd[threadIdx.x * 8 + e] = sd[e];
    __syncthreads();
    if (threadIdx.x < C4) {
        double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int q = 0; q < rpi; ++q)
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] += shd[(q * C4 + threadIdx.x) * 8 + e];
        float* o = p.part + (size_t)blockIdx.x * 2 * C + threadIdx.x * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = (float)t[e]; o[C + e] = (float)t[4 + e]; }
    }
}

// partials [groups][npg][2][C] -> coef [groups][2][C] = (sum_dzh/count, sum_dzh_xhat/count);
// dgamma/dbeta (+)= sums over all groups.
__global__ __launch_bounds__(FIN_T) void bn_bwd_finalize_kernel(const float* __restrict__ part, int npg, int groups, int C,
                                                               double count, float* coef, float* dgamma, float* dbeta,
                                                               int accum) {
    __shared__ double sh[2][FIN_RL][FIN_CL];
    const int cl = threadIdx.x % FIN_CL, rl = threadIdx.x / FIN_CL;
    const int c = blockIdx.x * FIN_CL + cl;
    double tg = 0.0, tb = 0.0;
    for (int g = 0; g < groups; ++g) {
        double s, s2;
        partial_colsum(part + (size_t)g * npg * 2 * C, npg, C, c, rl, sh, cl, s, s2);
        if (rl == 0 && c < C) {
            coef[(size_t)g * 2 * C + c] = (float)(s / count);
            coef[(size_t)g * 2 * C + C + c] = (float)(s2 / count);
            tb += s; tg += s2;
        }
    }
    if (rl == 0 && c < C) {
        if (dbeta) dbeta[c] = (accum ? dbeta[c] : 0.f) + (float)tb;
        if (dgamma) dgamma[c] = (accum ? dgamma[c] : 0.f) + (float)tg;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ z,
                                                           int ldz, const float* __restrict__ stat, const float* __restrict__ coef,
                                                           int C4, int64_t total4, int64_t rows_per_group, int relu,
                                                           float* __restrict__ dz, int lddz) {
    const int C = C4 * 4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
        const unsigned row = (unsigned)idx / (unsigned)C4;
        const int c = (int)((unsigned)idx - row * C4) * 4;
        const int g = (int)(row / (unsigned)rows_per_group);
        const float* st = stat + (size_t)g * 4 * C;
        const float* cf = coef + (size_t)g * 2 * C;
        const f32x4 d = *(const f32x4*)(dy + (size_t)row * lddy + c), zz = *(const f32x4*)(z + (size_t)row * ldz + c);
        const f32x4 mean = *(const f32x4*)(st + c), inv = *(const f32x4*)(st + C + c);
        const f32x4 sc = *(const f32x4*)(st + 2 * C + c), sh_ = *(const f32x4*)(st + 3 * C + c);
        const f32x4 c1 = *(const f32x4*)(cf + c), c2 = *(const f32x4*)(cf + C + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float yv = zz[e] * sc[e] + sh_[e];
            const float dd = (relu && !(yv > 0.f)) ? 0.f : d[e];
            o[e] = sc[e] * (dd - c1[e] - (zz[e] - mean[e]) * inv[e] * c2[e]);
        }
        *(f32x4*)(dz + (size_t)row * lddz + c) = o;
    }
}


// ------------------------------------------------------------------------------ BatchNorm with the finalize folded into the apply kernel (round 5)
// OPTIONAL (PICONS_BN_FUSED=1; off by default: measured no gain on the step, +0.1 ms of single-stream kernel time -- DESIGN.md 6, round 5).
// The finalize kernels are a handful of blocks between two streaming kernels on the step's dependency chain: 6 - 8 us alone, 20 - 26 us each
// in the four-lane step, where they wait for a free slot beside the other lanes' whole-CU GEMM blocks (17 + 15 such launches on lane 0 alone).
// For layers with few partial rows (the 28 x 28 layers: <= 256 per batch group) every block of the apply kernel instead reduces the partial
// rows of ITS 64 channels itself -- 16 row lanes x 16 float4 columns, doubles, fixed order; a few tens of KB from L2 -- and goes on to its
// rows.  Grid = (row blocks, 64-channel blocks, batch groups); the row block 0 of group 0 also writes what leaves the layer (stat / running
// statistics; d gamma / d beta), walking the other groups' partial rows for that.
constexpr int FA_CB = 64;        // channels per block
// sums of the partial rows [npg][2][C] over rows, for the channels cb * 64 .. + 63: valid on threads tid < 64 (channel cb * 64 + tid)
__device__ __forceinline__ void fa_partial_sums(const float* __restrict__ part, int npg, int C, int cb, int tid, double (*shd)[FA_CB][2], double& s, double& s2) {
    const int c4 = tid & 15, rl = tid >> 4, c = cb * FA_CB + c4 * 4;
    double a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    if (c < C) {
#pragma unroll 4
        for (int i = rl; i < npg; i += 16) {
            const f32x4 x = *(const f32x4*)(part + (size_t)i * 2 * C + c), y = *(const f32x4*)(part + (size_t)i * 2 * C + C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a[e] += (double)x[e]; b[e] += (double)y[e]; }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {          // the four row lanes of a wave (lane bits 4, 5), then the four waves through LDS
        a[e] += __shfl_xor(a[e], 16, 64); a[e] += __shfl_xor(a[e], 32, 64);
        b[e] += __shfl_xor(b[e], 16, 64); b[e] += __shfl_xor(b[e], 32, 64);
    }
    __syncthreads();                       // (a previous call's readers are done with shd)
    if ((tid & 63) < 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { shd[tid >> 6][c4 * 4 + e][0] = a[e]; shd[tid >> 6][c4 * 4 + e][1] = b[e]; }
    }
    __syncthreads();
    s = 0; s2 = 0;
    if (tid < FA_CB) {
        s = ((shd[0][tid][0] + shd[1][tid][0]) + shd[2][tid][0]) + shd[3][tid][0];
        s2 = ((shd[0][tid][1] + shd[1][tid][1]) + shd[2][tid][1]) + shd[3][tid][1];
    }
}

__global__ __launch_bounds__(256) void bn_fin_apply_kernel(const float* __restrict__ part, int npg, int groups, int C, double count,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float mom,
                                                           float* rmean, float* rvar, float* __restrict__ stat, const float* __restrict__ z, int ldz,
                                                           float* __restrict__ y, int ldy, int relu, int rows_per_group, int rows_per_block) {
    __shared__ double shd[4][FA_CB][2];
    __shared__ __attribute__((aligned(16))) float shs[2][FA_CB];
    const int tid = threadIdx.x, rb = blockIdx.x, cb = blockIdx.y, g = blockIdx.z;
    const int ch = cb * FA_CB + tid;                  // this thread's channel in the per-channel sections (tid < 64)
    double s, s2;
    fa_partial_sums(part + (size_t)g * npg * 2 * C, npg, C, cb, tid, shd, s, s2);
    double mean0 = 0, var0 = 0;
    if (tid < FA_CB && ch < C) {
        const double mean = s / count;
        double var = s2 / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const float invstd = (float)(1.0 / sqrt(var + (double)eps));
        const float sc = gamma[ch] * invstd, sh = beta[ch] - (float)mean * sc;
        shs[0][tid] = sc; shs[1][tid] = sh;
        if (rb == 0) {
            float* st = stat + (size_t)g * 4 * C;
            st[ch] = (float)mean; st[C + ch] = invstd; st[2 * C + ch] = sc; st[3 * C + ch] = sh;
        }
        mean0 = mean; var0 = var;
    }
    if (rb == 0 && g == 0 && rmean != nullptr) {      // block-uniform: running statistics over the batch groups IN ORDER (two forward passes)
        float rm = 0.f, rv = 0.f;
        if (tid < FA_CB && ch < C) { rm = rmean[ch]; rv = rvar[ch]; }
        for (int q = 0; q < groups; ++q) {
            double mean = mean0, var = var0;
            if (q > 0) {
                double t, t2;
                fa_partial_sums(part + (size_t)q * npg * 2 * C, npg, C, cb, tid, shd, t, t2);
                mean = t / count; var = t2 / count - mean * mean;
                if (var < 0.0) var = 0.0;
            }
            const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
            rm = (1.f - mom) * rm + mom * (float)mean;
            rv = (1.f - mom) * rv + mom * (float)unb;
        }
        if (tid < FA_CB && ch < C) { rmean[ch] = rm; rvar[ch] = rv; }
    }
    __syncthreads();
    const int c4 = tid & 15, rl = tid >> 4, c = cb * FA_CB + c4 * 4;
    if (c >= C) return;
    const f32x4 sc = *(const f32x4*)&shs[0][c4 * 4], sh = *(const f32x4*)&shs[1][c4 * 4];
    const int64_t r0 = (int64_t)g * rows_per_group + (int64_t)rb * rows_per_block;
    const int64_t r1 = min((int64_t)(g + 1) * rows_per_group, r0 + rows_per_block);
#pragma unroll 4
    for (int64_t r = r0 + rl; r < r1; r += 16) {
        const f32x4 v = *(const f32x4*)(z + r * ldz + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float t = v[e] * sc[e] + sh[e]; o[e] = relu ? fmaxf(t, 0.f) : t; }
        *(f32x4*)(y + r * ldy + c) = o;
    }
}

__global__ __launch_bounds__(256) void bn_bwd_fin_apply_kernel(const float* __restrict__ part, int npg, int groups, int C, double count,
                                                               const float* __restrict__ dy, int lddy, const float* __restrict__ z, int ldz,
                                                               const float* __restrict__ stat, int relu, float* __restrict__ dz, int lddz,
                                                               float* dgamma, float* dbeta, int accum, int rows_per_group, int rows_per_block) {
    __shared__ double shd[4][FA_CB][2];
    __shared__ __attribute__((aligned(16))) float shs[2][FA_CB];
    const int tid = threadIdx.x, rb = blockIdx.x, cb = blockIdx.y, g = blockIdx.z;
    const int ch = cb * FA_CB + tid;
    double s, s2;
    fa_partial_sums(part + (size_t)g * npg * 2 * C, npg, C, cb, tid, shd, s, s2);
    if (tid < FA_CB && ch < C) { shs[0][tid] = (float)(s / count); shs[1][tid] = (float)(s2 / count); }
    if (rb == 0 && g == 0) {                          // block-uniform: d beta / d gamma = the sums over every group, in group order
        double tb = s, tg = s2;
        for (int q = 1; q < groups; ++q) {
            double t, t2;
            fa_partial_sums(part + (size_t)q * npg * 2 * C, npg, C, cb, tid, shd, t, t2);
            tb += t; tg += t2;
        }
        if (tid < FA_CB && ch < C) {
            if (dbeta) dbeta[ch] = (accum ? dbeta[ch] : 0.f) + (float)tb;
            if (dgamma) dgamma[ch] = (accum ? dgamma[ch] : 0.f) + (float)tg;
        }
    }
    __syncthreads();
    const int c4 = tid & 15, rl = tid >> 4, c = cb * FA_CB + c4 * 4;
    if (c >= C) return;
    const f32x4 c1 = *(const f32x4*)&shs[0][c4 * 4], c2 = *(const f32x4*)&shs[1][c4 * 4];
    const float* st = stat + (size_t)g * 4 * C;
    const f32x4 mean = *(const f32x4*)(st + c), inv = *(const f32x4*)(st + C + c);
    const f32x4 sc = *(const f32x4*)(st + 2 * C + c), sh_ = *(const f32x4*)(st + 3 * C + c);
    const int64_t r0 = (int64_t)g * rows_per_group + (int64_t)rb * rows_per_block;
    const int64_t r1 = min((int64_t)(g + 1) * rows_per_group, r0 + rows_per_block);
#pragma unroll 4
    for (int64_t r = r0 + rl; r < r1; r += 16) {
        const f32x4 d = *(const f32x4*)(dy + r * lddy + c), zz = *(const f32x4*)(z + r * ldz + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float yv = zz[e] * sc[e] + sh_[e];
            const float dd = (relu && !(yv > 0.f)) ? 0.f : d[e];
            o[e] = sc[e] * (dd - c1[e] - (zz[e] - mean[e]) * inv[e] * c2[e]);
        }
        *(f32x4*)(dz + r * lddz + c) = o;
    }
}

// partial [nblk][2][C] -> dbias (+)=
__global__ __launch_bounds__(FIN_T) void colsum_finalize_kernel(const float* __restrict__ part, int nblk, int C, float* out, int accum) {
    __shared__ double sh[2][FIN_RL][FIN_CL];
    const int cl = threadIdx.x % FIN_CL, rl = threadIdx.x / FIN_CL;
    const int c = blockIdx.x * FIN_CL + cl;
    double s, s2;
    partial_colsum(part, nblk, C, c, rl, sh, cl, s, s2);
    if (rl == 0 && c < C) out[c] = (accum ? out[c] : 0.f) + (float)s;
}

__device__ __forceinline__ f32x4 act_bwd_of(const f32x4 d, const f32x4 yy, int act) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = d[e];
        if (act == PC_ACT_RELU) v = yy[e] > 0.f ? v : 0.f;
        else if (act == PC_ACT_SIGMOID) v = v * yy[e] * (1.f - yy[e]);
        o[e] = v;
    }
    return o;
}

__global__ __launch_bounds__(256) void act_bwd_apply_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                            int act, int C4, int64_t total4, float* __restrict__ dz, int lddz) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
        const size_t row = (unsigned)idx / (unsigned)C4;
        const int c = (int)((unsigned)idx - (unsigned)row * C4) * 4;
        const f32x4 d = *(const f32x4*)(dy + row * lddy + c), yy = *(const f32x4*)(y + row * ldy + c);
        *(f32x4*)(dz + row * lddz + c) = act_bwd_of(d, yy, act);
    }
}

// Bias gradient and dz in ONE pass over (dy, y): partial column sums [nblk][2][C] (second half unused, as colsum_finalize_kernel reads them) and,
// with WRITE, dz for every element read.  Block and thread partition, the runs of four rows flushed into double and the LDS combine are those of
// colreduce_kernel, so the sums are the same bits whether dz is written or not; four rows are in flight per thread (eight 16-byte loads).
// dz may be dy (each element is read and written by one thread, read first).
template <bool WRITE>
__global__ __launch_bounds__(256) void act_bwd_reduce_kernel(const float* dy, int lddy, const float* __restrict__ y, int ldy, int act, int C4, int64_t rows,
                                                             int64_t rows_per_block, float* dz, int lddz, float* __restrict__ part) {
    const int C = C4 * 4;
    const int rpi = 256 / C4;                       // rows per iteration
    const int c4 = threadIdx.x % C4, rl = threadIdx.x / C4;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    double sd[4] = {0, 0, 0, 0};
    if (rl < rpi) {
        const int c = c4 * 4;
        int64_t r = r0 + rl;
        for (; r + 3 * (int64_t)rpi < r1; r += 4 * (int64_t)rpi) {
            f32x4 d[4], yy[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                d[u] = *(const f32x4*)(dy + (r + (int64_t)u * rpi) * lddy + c);
                yy[u] = *(const f32x4*)(y + (r + (int64_t)u * rpi) * ldy + c);
            }
            float s[4] = {0, 0, 0, 0};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 o = act_bwd_of(d[u], yy[u], act);
                if (WRITE) *(f32x4*)(dz + (r + (int64_t)u * rpi) * lddz + c) = o;
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += o[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) sd[e] += (double)s[e];
        }
        float s[4] = {0, 0, 0, 0};                  // the last, shorter run
        for (; r < r1; r += rpi) {
            const f32x4 o = act_bwd_of(*(const f32x4*)(dy + r * lddy + c), *(const f32x4*)(y + r * ldy + c), act);
            if (WRITE) *(f32x4*)(dz + r * lddz + c) = o;
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += o[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sd[e] += (double)s[e];
    }
    __shared__ double shd[256 * 4];
#pragma unroll
    for (int e = 0; e < 4; ++e) shd[threadIdx.x * 4 + e] = sd[e];
    __syncthreads();
    if (threadIdx.x < C4) {
        double t[4] = {0, 0, 0, 0};
        for (int q = 0; q < rpi; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += shd[(q * C4 + threadIdx.x) * 4 + e];
        float* o = part + (size_t)blockIdx.x * 2 * C + threadIdx.x * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = (float)t[e]; o[C + e] = 0.f; }
    }
}

// ------------------------------------------------------------------------------ max pool
// Work order of both directions: a block owns a contiguous run of `ppb` positions (output positions forward, input positions backward) with all
// their channels, and the block that owns run i is the one whose xcd_remap id is i.  A line of the other tensor is needed by up to 27 positions
// of neighbouring rows and planes; blocks that run at the same time on one XCD then sweep adjacent rows, and that XCD's L2 serves the overlap
// (dealt out round-robin, the rows around a line ran on all eight XCDs, whose L2s are private).  The remap moves work between blocks and nothing else.
// The windows the planner emits are compile-time forms <KT, KH, KW, ST, SH, SW>: the taps of one temporal plane are loaded together (clamped
// addresses for the spatial padding, no load for a padded plane) and then compared / added in order.  KT = 0: any window, from the descriptor.
constexpr int POOL_ITEMS = 1024;                    // float4 items per block: four per thread

template <int KT, int KH, int KW, int ST, int SH, int SW>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const pc_pool_desc d, const float* __restrict__ x, float* __restrict__ y,
                                                          uint8_t* __restrict__ am, unsigned npos, unsigned ppb) {
    const unsigned C4 = (unsigned)d.C / 4;
    const unsigned p0 = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x) * ppb;
    if (p0 >= npos) return;
    const unsigned items = (min(npos, p0 + ppb) - p0) * C4;
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        unsigned pos = p0 + i / C4;
        const int c = (int)(i % C4) * 4;
        const size_t opos = pos;
        const int wo = (int)(pos % (unsigned)d.Wo); pos /= (unsigned)d.Wo;
        const int ho = (int)(pos % (unsigned)d.Ho); pos /= (unsigned)d.Ho;
        const int to = (int)(pos % (unsigned)d.To); const int n = (int)(pos / (unsigned)d.To);
        f32x4 best = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bi[4] = {255, 255, 255, 255};
        if constexpr (KT == 0) {
            int tap = 0;
            for (int a = 0; a < d.k[0]; ++a) {
                const int t = to * d.s[0] - d.padf[0] + a;
                for (int b = 0; b < d.k[1]; ++b) {
                    const int h = ho * d.s[1] - d.padf[1] + b;
                    for (int cc = 0; cc < d.k[2]; ++cc, ++tap) {
                        const int w = wo * d.s[2] - d.padf[2] + cc;
                        const bool inb = (unsigned)t < (unsigned)d.Ti && (unsigned)h < (unsigned)d.Hi && (unsigned)w < (unsigned)d.Wi;
                        f32x4 v = {0.f, 0.f, 0.f, 0.f};   // F.pad zero (pytorch_i3d.py:44)
                        if (inb) v = *(const f32x4*)(x + ((size_t)((n * d.Ti + t) * d.Hi + h) * d.Wi + w) * d.ldi + c);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (v[e] > best[e]) { best[e] = v[e]; bi[e] = inb ? tap : 255; }
                    }
                }
            }
        } else {
            const int h0 = ho * SH - d.padf[1], w0 = wo * SW - d.padf[2];
#pragma unroll
            for (int a = 0; a < KT; ++a) {
                const int t = to * ST - d.padf[0] + a;
                if ((unsigned)t >= (unsigned)d.Ti) {       // a plane of padding: nine zeros with index 255, of which only the first can win
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (0.f > best[e]) { best[e] = 0.f; bi[e] = 255; }
                    continue;
                }
                f32x4 v[KH * KW];
                const float* xp = x + (size_t)(n * d.Ti + t) * d.Hi * d.Wi * d.ldi + c;
#pragma unroll
                for (int b = 0; b < KH; ++b)
#pragma unroll
                    for (int cc = 0; cc < KW; ++cc) {
                        const int h = min(max(h0 + b, 0), d.Hi - 1), w = min(max(w0 + cc, 0), d.Wi - 1);
                        v[b * KW + cc] = *(const f32x4*)(xp + ((size_t)h * d.Wi + w) * d.ldi);
                    }
#pragma unroll
                for (int b = 0; b < KH; ++b)
#pragma unroll
                    for (int cc = 0; cc < KW; ++cc) {
                        const bool inb = (unsigned)(h0 + b) < (unsigned)d.Hi && (unsigned)(w0 + cc) < (unsigned)d.Wi;
                        const int tap = (a * KH + b) * KW + cc;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float u = inb ? v[b * KW + cc][e] : 0.f;   // F.pad zero (pytorch_i3d.py:44)
                            if (u > best[e]) { best[e] = u; bi[e] = inb ? tap : 255; }
                        }
                    }
            }
        }
        *(f32x4*)(y + opos * d.ldo + c) = best;
        *(uchar4*)(am + opos * d.C + c) = make_uchar4(bi[0], bi[1], bi[2], bi[3]);
    }
}

template <int KT, int KH, int KW, int ST, int SH, int SW>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const pc_pool_desc d, const float* __restrict__ dy, const uint8_t* __restrict__ am,
                                                          float* __restrict__ dx, int accum, unsigned npos, unsigned ppb) {
    const unsigned C4 = (unsigned)d.C / 4;
    const unsigned p0 = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x) * ppb;
    if (p0 >= npos) return;
    const unsigned items = (min(npos, p0 + ppb) - p0) * C4;
    const int K[3] = {KT ? KT : d.k[0], KT ? KH : d.k[1], KT ? KW : d.k[2]}, S[3] = {KT ? ST : d.s[0], KT ? SH : d.s[1], KT ? SW : d.s[2]};
    for (unsigned i = threadIdx.x; i < items; i += 256) {
        unsigned pos = p0 + i / C4;
        const int c = (int)(i % C4) * 4;
        const size_t ipos = pos;
        const int w = (int)(pos % (unsigned)d.Wi); pos /= (unsigned)d.Wi;
        const int h = (int)(pos % (unsigned)d.Hi); pos /= (unsigned)d.Hi;
        const int t = (int)(pos % (unsigned)d.Ti); const int n = (int)(pos / (unsigned)d.Ti);
        float* o = dx + ipos * d.ldi + c;
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (accum) old = *(const f32x4*)o;
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        // windows that cover this input position: per dimension the outputs o with 0 <= x + padf - o*s < k
        int lo[3], hi[3];
        const int xs[3] = {t, h, w}, Os[3] = {d.To, d.Ho, d.Wo};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int top = xs[q] + d.padf[q], bot = top - K[q] + 1;
            hi[q] = min(top / S[q], Os[q] - 1);
            lo[q] = bot <= 0 ? 0 : (bot + S[q] - 1) / S[q];
        }
        if constexpr (KT == 0) {
            for (int to = lo[0]; to <= hi[0]; ++to) {
                const int a = t + d.padf[0] - to * S[0];
                for (int ho = lo[1]; ho <= hi[1]; ++ho) {
                    const int b = h + d.padf[1] - ho * S[1];
                    for (int wo = lo[2]; wo <= hi[2]; ++wo) {
                        const int tap = (a * K[1] + b) * K[2] + (w + d.padf[2] - wo * S[2]);
                        const size_t op = (size_t)((n * d.To + to) * d.Ho + ho) * d.Wo + wo;
                        const uchar4 ix = *(const uchar4*)(am + op * d.C + c);
                        const f32x4 v = *(const f32x4*)(dy + op * d.ldo + c);
                        if (ix.x == tap) g[0] += v[0];
                        if (ix.y == tap) g[1] += v[1];
                        if (ix.z == tap) g[2] += v[2];
                        if (ix.w == tap) g[3] += v[3];
                    }
                }
            }
        } else {
            // at most ceil(k / s) windows per dimension: those of one output plane are loaded together (clamped: a window past hi is not added)
            constexpr int MT = (KT + ST - 1) / ST, MH = (KH + SH - 1) / SH, MW = (KW + SW - 1) / SW;
#pragma unroll
            for (int jt = 0; jt < MT; ++jt) {
                const int to = lo[0] + jt;
                if (to > hi[0]) break;
                const int a = t + d.padf[0] - to * ST;
                uchar4 ix[MH * MW];
                f32x4 v[MH * MW];
#pragma unroll
                for (int jh = 0; jh < MH; ++jh)
#pragma unroll
                    for (int jw = 0; jw < MW; ++jw) {
                        const int ho = min(lo[1] + jh, d.Ho - 1), wo = min(lo[2] + jw, d.Wo - 1);
                        const size_t op = (size_t)((n * d.To + to) * d.Ho + ho) * d.Wo + wo;
                        ix[jh * MW + jw] = *(const uchar4*)(am + op * d.C + c);
                        v[jh * MW + jw] = *(const f32x4*)(dy + op * d.ldo + c);
                    }
#pragma unroll
                for (int jh = 0; jh < MH; ++jh)
#pragma unroll
                    for (int jw = 0; jw < MW; ++jw) {
                        const int ho = lo[1] + jh, wo = lo[2] + jw;
                        const int tap = (ho <= hi[1] && wo <= hi[2]) ? (a * KH + (h + d.padf[1] - ho * SH)) * KW + (w + d.padf[2] - wo * SW) : 256;
                        const uchar4 q = ix[jh * MW + jw];
                        const f32x4 u = v[jh * MW + jw];
                        if (q.x == tap) g[0] += u[0];
                        if (q.y == tap) g[1] += u[1];
                        if (q.z == tap) g[2] += u[2];
                        if (q.w == tap) g[3] += u[3];
                    }
            }
        }
        if (accum) g += old;
        *(f32x4*)o = g;
    }
}

// The 3x3x3 windows with stride 1 along h and w (ST = 1 or 2 along t): a thread owns a register tile of four adjacent positions times four
// channels -- forward 2 x 2 outputs (h x w), backward POOL_WT input positions along w -- one (tile, channel quad) item per thread, a block
// 256 consecutive items (tiles in row order, channels fastest), blocks in the same XCD-local order.  The positions of a tile share taps: a
// temporal plane is loaded once for all four (forward 4 x 4 = 16 quads, backward 3 x 6 = 18 (argmax, dy) pairs, instead of 36) and then
// compared / added per position in exactly the order of the kernels above -- forward (kt, kh, kw) with a strict `>`, a padding tap 0 with
// index 255, a padded plane one compare; backward ascending (to, ho, wo), the old dx last.  Lanes stay channel-contiguous, so every access
// is a coalesced 16-byte one.  A tile that reaches past the end of a row (or, forward, past the last row) loads clamped addresses there
// and stores nothing.
constexpr int POOL_WT = 4;

template <int ST>
__global__ __launch_bounds__(256, 4) void maxpool333_fwd_tile_kernel(const pc_pool_desc d, const float* __restrict__ x, float* __restrict__ y,
                                                                     uint8_t* __restrict__ am, unsigned nitems) {
    const unsigned C4 = (unsigned)d.C / 4, tw = ((unsigned)d.Wo + 1) / 2, th = ((unsigned)d.Ho + 1) / 2;
    const unsigned i = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x) * 256 + threadIdx.x;
    if (i < nitems) {
        unsigned q = i / C4;
        const int c = (int)(i % C4) * 4;
        const int wo0 = (int)(q % tw) * 2; q /= tw;
        const int ho0 = (int)(q % th) * 2; q /= th;
        const int to = (int)(q % (unsigned)d.To); const int n = (int)(q / (unsigned)d.To);
        f32x4 best[4];                                     // position u = 2 * (row of the tile) + column
        unsigned bi[4];                                    // the winning tap of each of the four channels, one byte each
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            best[u] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            bi[u] = 0xFFFFFFFFu;
        }
        const int h0 = ho0 - d.padf[1], w0 = wo0 - d.padf[2];
#pragma unroll 1
        for (int a = 0; a < 3; ++a) {
            const int t = to * ST - d.padf[0] + a;
            if ((unsigned)t >= (unsigned)d.Ti) {       // a plane of padding: nine zeros with index 255, of which only the first can win
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (0.f > best[u][e]) { best[u][e] = 0.f; bi[u] |= 0xFFu << (8 * e); }
                continue;
            }
            // Registers: the taps take 64 and the running maxima 20.  An address is a 32-bit byte offset from x, one register (the host sends
            // inputs of 4 GB and more to the kernel above), and is worked out here, per plane: the asm keeps the compiler from holding the
            // sixteen in-plane offsets in registers across the plane loop
            f32x4 v[4][4];
            const unsigned pb = ((unsigned)((n * d.Ti + t) * d.Hi) * (unsigned)d.Wi * (unsigned)d.ldi + (unsigned)c) * 4u;
            int h0a = h0, w0a = w0;
            asm volatile("" : "+v"(h0a), "+v"(w0a));
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int h = min(max(h0a + r, 0), d.Hi - 1), w = min(max(w0a + j, 0), d.Wi - 1);
                    v[r][j] = *(const f32x4*)((const char*)x + (pb + (unsigned)(h * d.Wi + w) * (unsigned)d.ldi * 4u));
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!((unsigned)(h0 + r) < (unsigned)d.Hi && (unsigned)(w0 + j) < (unsigned)d.Wi)) v[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};   // F.pad zero (pytorch_i3d.py:44)
            const unsigned tap0 = (unsigned)a * 9u;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int b = 0; b < 3; ++b)
#pragma unroll
                    for (int cc = 0; cc < 3; ++cc) {
                        const unsigned tap4 = (tap0 + (unsigned)(b * 3 + cc)) * 0x01010101u;
                        const f32x4 z = v[u / 2 + b][u % 2 + cc];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const unsigned m = 0xFFu << (8 * e);
                            if (z[e] > best[u][e]) { best[u][e] = z[e]; bi[u] = (bi[u] & ~m) | (tap4 & m); }
                        }
                    }
        }
        // a winning tap that lies in the spatial padding reads 255: bit (kh, kw) of `in9` says whether that tap of position u is inside, the
        // same for the three planes (a padded plane has written 255 itself, and 255 & 31 = 31 is a clear bit)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ho = ho0 + u / 2, wo = wo0 + u % 2;
            unsigned in9 = 0;
#pragma unroll
            for (int b = 0; b < 3; ++b)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    if ((unsigned)(h0 + u / 2 + b) < (unsigned)d.Hi && (unsigned)(w0 + u % 2 + cc) < (unsigned)d.Wi) in9 |= 1u << (b * 3 + cc);
            const unsigned in27 = in9 | in9 << 9 | in9 << 18;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (!(in27 >> ((bi[u] >> (8 * e)) & 31u) & 1u)) bi[u] |= 0xFFu << (8 * e);
            if (ho < d.Ho && wo < d.Wo) {
                const size_t opos = (size_t)((n * d.To + to) * d.Ho + ho) * d.Wo + wo;
                *(f32x4*)(y + opos * d.ldo + c) = best[u];
                *(unsigned*)(am + opos * d.C + c) = bi[u];
            }
        }
    }
}

template <int ST, int WT>
__global__ __launch_bounds__(256, 4) void maxpool333_bwd_tile_kernel(const pc_pool_desc d, const float* __restrict__ dy, const uint8_t* __restrict__ am,
                                                                     float* __restrict__ dx, int accum, unsigned nitems) {
    const unsigned C4 = (unsigned)d.C / 4, tw = ((unsigned)d.Wi + WT - 1) / WT;
    const unsigned i = (unsigned)xcd_remap((int)blockIdx.x, (int)gridDim.x) * 256 + threadIdx.x;
    if (i < nitems) {
        unsigned q = i / C4;
        const int c = (int)(i % C4) * 4;
        const int w0 = (int)(q % tw) * WT; q /= tw;
        const int h = (int)(q % (unsigned)d.Hi); q /= (unsigned)d.Hi;
        const int t = (int)(q % (unsigned)d.Ti); const int n = (int)(q / (unsigned)d.Ti);
        f32x4 g[WT];
#pragma unroll
        for (int u = 0; u < WT; ++u) g[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        // windows that cover an input position: per dimension the outputs o with 0 <= x + padf - o*s < 3.  Along h and w (stride 1) those are
        // o = x + padf - 2 .. x + padf where they exist: rows hb .. hb + 2 and, for the whole tile, columns wb .. wb + WT + 1
        const int top = t + d.padf[0], bot = top - 2;
        const int thi = min(top / ST, d.To - 1), tlo = bot <= 0 ? 0 : (bot + ST - 1) / ST;
        const int hb = h + d.padf[1] - 2, wb = w0 + d.padf[2] - 2;
        constexpr int MT = (3 + ST - 1) / ST;
#pragma unroll 1
        for (int jt = 0; jt < MT; ++jt) {
            const int to = tlo + jt;
            if (to > thi) break;
            const int a = top - to * ST;
            uchar4 ix[3][WT + 2];
            f32x4 v[3][WT + 2];
#pragma unroll
            for (int jh = 0; jh < 3; ++jh)
#pragma unroll
                for (int j = 0; j < WT + 2; ++j) {
                    const int ho = min(max(hb + jh, 0), d.Ho - 1), wo = min(max(wb + j, 0), d.Wo - 1);
                    const size_t op = (size_t)((n * d.To + to) * d.Ho + ho) * d.Wo + wo;
                    ix[jh][j] = *(const uchar4*)(am + op * d.C + c);
                    v[jh][j] = *(const f32x4*)(dy + op * d.ldo + c);
                }
#pragma unroll
            for (int jh = 0; jh < 3; ++jh)                 // row by row: every position still sees its windows in (ho, wo) order
#pragma unroll
                for (int u = 0; u < WT; ++u)
#pragma unroll
                    for (int jw = 0; jw < 3; ++jw) {          // output (hb + jh, wb + u + jw) holds this position as tap (a, 2 - jh, 2 - jw)
                        const bool ok = (unsigned)(hb + jh) < (unsigned)d.Ho && (unsigned)(wb + u + jw) < (unsigned)d.Wo;
                        const int tap = ok ? (a * 3 + (2 - jh)) * 3 + (2 - jw) : 256;
                        const uchar4 k = ix[jh][u + jw];
                        const f32x4 z = v[jh][u + jw];
                        if (k.x == tap) g[u][0] += z[0];
                        if (k.y == tap) g[u][1] += z[1];
                        if (k.z == tap) g[u][2] += z[2];
                        if (k.w == tap) g[u][3] += z[3];
                    }
        }
        float* o = dx + ((size_t)((n * d.Ti + t) * d.Hi + h) * d.Wi + w0) * d.ldi + c;
#pragma unroll
        for (int u = 0; u < WT; ++u)
            if (w0 + u < d.Wi) {
                if (accum) g[u] += *(const f32x4*)(o + (size_t)u * d.ldi);
                *(f32x4*)(o + (size_t)u * d.ldi) = g[u];
            }
    }
}

// ------------------------------------------------------------------------------ misc elementwise
__global__ __launch_bounds__(256) void chscale_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ sc, int64_t pos_per_n,
                                                      int C4, int64_t total4, float* __restrict__ y, int ldy, int accum) {
    const int C = C4 * 4;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
        const size_t row = (unsigned)idx / (unsigned)C4;
        const int c = (int)((unsigned)idx - (unsigned)row * C4) * 4;
        const size_t n = (unsigned)row / (unsigned)pos_per_n;
        const f32x4 v = *(const f32x4*)(x + row * ldx + c), s = *(const f32x4*)(sc + n * C + c);
        f32x4 o = v * s;
        float* q = y + row * ldy + c;
        if (accum) o += *(const f32x4*)q;
        *(f32x4*)q = o;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void to_ndhwc_kernel(const T* __restrict__ src, int N, int C, int64_t thw, int W, int Cpad, int flipw,
                                                       float* __restrict__ dst) {
    const int64_t total = (int64_t)N * thw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t n = idx / thw, pos = idx - n * thw;
        int64_t sp = pos;
        if (flipw) { const int w = (int)(pos % W); sp = pos - w + (W - 1 - w); }
        if (Cpad == 4) {          // the RGB clip (3 -> 4 channels): one 16-byte store per position instead of four 4-byte stores at a 16-byte stride
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = c < C ? (float)src[(n * C + c) * thw + sp] : 0.f;
            *(f32x4*)(dst + idx * 4) = v;
            continue;
        }
        for (int c = 0; c < Cpad; ++c)
            dst[idx * Cpad + c] = c < C ? (float)src[(n * C + c) * thw + sp] : 0.f;
    }
}

__global__ __launch_bounds__(256) void to_ncdhw_kernel(const float* __restrict__ src, int ld, int N, int C, int64_t thw, float* __restrict__ dst) {
    const int64_t total = (int64_t)N * C * thw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t pos = idx % thw; const int64_t nc = idx / thw;
        const int c = (int)(nc % C); const int64_t n = nc / C;
        dst[idx] = src[(n * thw + pos) * ld + c];
    }
}

// dst[b][c][r] (+)= src[b][r][c]   (32x32 LDS tiles; used for every weight / weight-grad re-layout)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ src, int R, int Cc, int64_t sbs, int sld,
                                                        float* __restrict__ dst, int64_t dbs, int dld, int accum) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < Cc) ? src[(size_t)b * sbs + (size_t)r * sld + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < Cc && r < R) {
            float* o = dst + (size_t)b * dbs + (size_t)c * dld + r;
            *o = (accum ? *o : 0.f) + tile[tx][i];
        }
    }
}

// Many independent transposes in one launch (the ~160 weight re-layouts at the start of every step): the jobs travel
// by value in the kernel arguments, a block finds its job from the tile prefix sums.
constexpr int TM_JOBS = 40;
struct TJobK { const float* src; float* dst; long long sbs, dbs, sst; int R, Cc, sld, dld, accum, tiles_c, tiles_rc, nsl, tr, pad_; };
struct TPack { TJobK j[TM_JOBS]; int first[TM_JOBS + 1]; int n; };

__global__ __launch_bounds__(256) void transpose_multi_kernel(const TPack pk) {
    __shared__ float tile[32][33];
    int k = 0;
    while (k + 1 < pk.n && (int)blockIdx.x >= pk.first[k + 1]) ++k;
    const TJobK& J = pk.j[k];
    const int t = blockIdx.x - pk.first[k];
    const int b = t / J.tiles_rc, rem = t - b * J.tiles_rc;
    // tr = rows of a tile: 32, or 8 for a job that sums many K-slice images (four times the blocks, one element per thread)
    const int r0 = (rem / J.tiles_c) * J.tr, c0 = (rem % J.tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (J.nsl <= 1) {
        for (int i = ty; i < J.tr; i += 8) {
            const int r = r0 + i, c = c0 + tx;
            tile[i][tx] = (r < J.R && c < J.Cc) ? J.src[(size_t)b * J.sbs + (size_t)r * J.sld + c] : 0.f;
        }
    } else {
        // src is nsl K-slice images of a split-K weight gradient, sst floats apart (pc_conv_wgrad with ws_slices): added in slice
        // order -- the sum does not depend on which block finished when (no atomics anywhere on the way).  A thread owns four consecutive
        // columns of one row (one 16-byte load per image, sixteen in flight); J.tr = 8: a quarter of the threads' rows, four times the blocks
        const int i = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
        if (i < J.tr) {
            const int r = r0 + i, c = c0 + c4;
            f32x4 sum = {0.f, 0.f, 0.f, 0.f};
            if (r < J.R && c < J.Cc) {                     // src_ld % 4 == 0 (checked by the host): the quad lies inside the row (columns >= Cc are padding, never stored)
                const f32x4* q = (const f32x4*)(J.src + (size_t)b * J.sbs + (size_t)r * J.sld + c);
                const size_t st4 = (size_t)J.sst / 4;
                int k = 0;
                for (; k + 16 <= J.nsl; k += 16) {
                    f32x4 t[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) t[u] = q[(size_t)(k + u) * st4];
#pragma unroll
                    for (int u = 0; u < 16; ++u) sum += t[u];
                }
                for (; k + 4 <= J.nsl; k += 4) {
                    f32x4 t[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) t[u] = q[(size_t)(k + u) * st4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) sum += t[u];
                }
                for (; k < J.nsl; ++k) sum += q[(size_t)k * st4];
            }
            tile[i][c4] = sum[0]; tile[i][c4 + 1] = sum[1]; tile[i][c4 + 2] = sum[2]; tile[i][c4 + 3] = sum[3];
        }
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (tx < J.tr && c < J.Cc && r < J.R) {
            float* o = J.dst + (size_t)b * J.dbs + (size_t)c * J.dld + r;
            *o = (J.accum ? *o : 0.f) + tile[tx][i];
        }
    }
}

// The jobs of a pc_transpose_multi call that move rows, not tiles.  Two kinds, both with unit stride on the source side:
//   C == 1 without slices and src_ld == 1 (the forward re-layout of a 1x1x1 weight): dst[b][r] (+)= src[b][r], a copy per batch;
//   R == 1 (the gradient of such a weight, with its K-slice images): dst[b][c * dst_ld] (+)= sum over the images of src[b][c].
// Through the tile kernel these launch a block per 32 floats, and in the sliced ones 8 of its 256 threads do the sums.  Here a job is
// batch rows of L floats, a thread owns one quad of one row, a block 256 consecutive quads of the job (rows are not padded to the block),
// and a sliced job has sixteen 16-byte loads in flight in every thread.  The value is the tile kernel's, expression for expression:
// without slices the source element itself, with slices a sum that starts from zero and adds the images in ascending order; then
// (accum ? old : 0) + value.  vld / vst: whether the rows allow 16-byte loads / stores (set by the host from the pointers and strides);
// a quad that reaches past L stores its elements one by one.
struct RJobK { const float* src; float* dst; long long sbs, dbs, sst; int batch, L, dstep, accum, nsl, qpr, vld, vst; };
struct RPack { RJobK j[TM_JOBS]; int first[TM_JOBS + 1]; int n; };

__global__ __launch_bounds__(256) void relayout_rows_kernel(const RPack pk) {
    int k = 0;
    while (k + 1 < pk.n && (int)blockIdx.x >= pk.first[k + 1]) ++k;
    const RJobK& J = pk.j[k];
    const long long gq = (long long)((int)blockIdx.x - pk.first[k]) * 256 + threadIdx.x;
    const long long b = gq / J.qpr;
    if (b >= J.batch) return;
    const int c = (int)(gq - b * J.qpr) * 4;
    const float* s = J.src + b * J.sbs + c;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (J.nsl <= 1) {
        if (J.vld) v = *(const f32x4*)s;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < J.L) v[e] = s[e];
        }
    } else {                                               // the host has checked alignment and that the quad lies inside the row (L <= src_ld)
        const f32x4* q = (const f32x4*)s;
        const size_t st4 = (size_t)J.sst / 4;
        int i = 0;
        for (; i + 16 <= J.nsl; i += 16) {
            f32x4 t[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) t[u] = q[(size_t)(i + u) * st4];
#pragma unroll
            for (int u = 0; u < 16; ++u) v += t[u];
        }
        for (; i + 4 <= J.nsl; i += 4) {
            f32x4 t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = q[(size_t)(i + u) * st4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v += t[u];
        }
        for (; i < J.nsl; ++i) v += q[(size_t)i * st4];
    }
    float* o = J.dst + b * J.dbs + (long long)c * J.dstep;
    if (J.vst && c + 4 <= J.L) {
        f32x4 old = {0.f, 0.f, 0.f, 0.f};
        if (J.accum) old = *(const f32x4*)o;
        *(f32x4*)o = old + v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < J.L) {
                float* p = o + (long long)e * J.dstep;
                *p = (J.accum ? *p : 0.f) + v[e];
            }
    }
}

// K-slice images of an ordered split-K weight gradient, folded in place: image g * group of every group of `group` consecutive images
// becomes the sum of the group's images, added in slice order.  One thread per float4 of the image and group: `group` independent loads.
template <int GROUP>
__global__ __launch_bounds__(256) void slices_fold_kernel(float* __restrict__ ws, int64_t image4, int nslices, int64_t total) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t e = idx % image4; const int g = (int)(idx / image4);
        float4* base = (float4*)ws + (int64_t)g * GROUP * image4 + e;
        const int n = min(GROUP, nslices - g * GROUP);
        float4 t[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k) if (k < n) t[k] = base[(int64_t)k * image4];
        float4 sum = t[0];
#pragma unroll
        for (int k = 1; k < GROUP; ++k) if (k < n) { sum.x += t[k].x; sum.y += t[k].y; sum.z += t[k].z; sum.w += t[k].w; }
        base[0] = sum;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float* p, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}
__global__ __launch_bounds__(256) void axpy_kernel(float* y, const float* x, int64_t n, float a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] += a * x[i];
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   int64_t n, float lr_bc1, float b1, float b2, float omb1, float omb2, float eps, float inv_sqrt_bc2,
                                                   float gscale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i] * gscale;
        const float mi = b1 * m[i] + omb1 * gi;
        const float vi = b2 * v[i] + omb2 * gi * gi;
        m[i] = mi; v[i] = vi;
        p[i] -= lr_bc1 * mi / (sqrtf(vi) * inv_sqrt_bc2 + eps);
    }
}

// dx[n,h,w,c] (+)= sum_{b,c'} cols[n, h-b, w-c'][(b*KW+c')*C + c]   (valid (h-b, w-c') only): the gather half of an exact
// 'full' 2-D correlation computed as GEMM (cols = dY x W^T, one column block per tap) + col2im.
__global__ __launch_bounds__(256) void col2im_kernel(const float* __restrict__ cols, int N, int Ho, int Wo, int KH, int KW, int C4,
                                                     float* __restrict__ dx, int lddx, int accum, int64_t total4) {
    const int Hi = Ho + KH - 1, Wi = Wo + KW - 1, C = C4 * 4;
    const size_t ldc = (size_t)KH * KW * C;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (int64_t)gridDim.x * 256) {
        int64_t pos = idx / C4;
        const int c = (int)(idx - pos * C4) * 4;
        const int64_t ipos = pos;
        const int w = (int)(pos % Wi); pos /= Wi;
        const int h = (int)(pos % Hi); const int n = (int)(pos / Hi);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int b0 = max(0, h - (Ho - 1)), b1 = min(KH - 1, h), c0 = max(0, w - (Wo - 1)), c1 = min(KW - 1, w);
        for (int b = b0; b <= b1; ++b)
            for (int cc = c0; cc <= c1; ++cc) {
                const size_t op = (size_t)((n * Ho + (h - b)) * Wo + (w - cc));
                acc += *(const f32x4*)(cols + op * ldc + (size_t)(b * KW + cc) * C + c);
            }
        float* o = dx + ipos * lddx + c;
        if (accum) acc += *(const f32x4*)o;
        *(f32x4*)o = acc;
    }
}

inline int grid_for(int64_t n, int per_thread = 1) {
    int64_t b = (n + 256ll * per_thread - 1) / (256ll * per_thread);
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (int)b;
}
inline int pool_blocks(int64_t total4) { return total4 > POOL_ITEMS ? (int)((total4 + POOL_ITEMS - 1) / POOL_ITEMS) : 1; }
// items of the register-tile pool kernels: `rows` rows of W positions cut into tiles of POOL_WT, times C4 channel quads (never more than total4)
inline int64_t pool_tile_items(int64_t rows, int W, int C4) { return rows * ((W + POOL_WT - 1) / POOL_WT) * C4; }
// the forward tile kernel addresses its input with 32-bit byte offsets
inline bool pool_in_4g(const pc_pool_desc* d) { return (int64_t)d->N * d->Ti * d->Hi * d->Wi * d->ldi * 4 < (1ll << 32); }
// which compile-time window / stride form of the pool kernels a descriptor takes (0: the generic body)
inline int pool_form(const pc_pool_desc* d) {
    const auto is = [](const int32_t* v, int a, int b, int c) { return v[0] == a && v[1] == b && v[2] == c; };
    if (is(d->k, 1, 3, 3) && is(d->s, 1, 2, 2)) return 1;
    if (is(d->k, 3, 3, 3) && is(d->s, 2, 1, 1)) return 2;
    if (is(d->k, 3, 3, 3) && is(d->s, 1, 1, 1)) return 3;
    return 0;
}
// the double nearest to the shortest decimal string that converts back to exactly this float (0.999f -> 0.999, 0.9f -> 0.9)
inline double pc_decimal_of_float(float x) {
    char buf[40];
    for (int prec = 1; prec <= 9; ++prec) {
        snprintf(buf, sizeof(buf), "%.*g", prec, (double)x);
        const double d = strtod(buf, nullptr);
        if ((float)d == x) return d;
    }
    return (double)x;
}
inline int64_t red_rows_per_block(int64_t rows) {
    int64_t r = (rows + 1023) / 1024;
    if (r < 32) r = 32;
    return r;
}

}  // namespace

// ================================================================================ C ABI
extern "C" int64_t pc_bn_finalize_ws_floats(int nparts_per_group, int groups, int C) {
    return nparts_per_group >= 512 ? (int64_t)groups * FIN_S * 2 * C * 2 + 2 : 0;       // doubles, + room to align
}

extern "C" int pc_bn_finalize_ws(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group,
                                 const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                                 float* running_var, float* stat, float* ws, pc_stream s) {
    PC_CHECK_ARG(part && gamma && beta && stat && groups >= 1 && C > 0, "pc_bn_finalize: bad args");
    if (ws && nparts_per_group >= 512) {
        double* w = (double*)(((uintptr_t)ws + 7) & ~(uintptr_t)7);
        hipLaunchKernelGGL(bn_partial_reduce_kernel, dim3(cdiv(C, FIN_CL), FIN_S, groups), dim3(FIN_T), 0, (hipStream_t)s, part, nparts_per_group, C, w);
        hipLaunchKernelGGL(bn_finalize_kernel<double>, dim3(cdiv(C, FIN_CL)), dim3(FIN_T), 0, (hipStream_t)s, (const double*)w, FIN_S, groups, C,
                           (double)count_per_group, gamma, beta, eps, momentum, running_mean, running_var, stat);
    } else {
        hipLaunchKernelGGL(bn_finalize_kernel<float>, dim3(cdiv(C, FIN_CL)), dim3(FIN_T), 0, (hipStream_t)s, part, nparts_per_group, groups, C,
                           (double)count_per_group, gamma, beta, eps, momentum, running_mean, running_var, stat);
    }
    PC_CHECK_LAUNCH("bn_finalize");
    return PC_OK;
}

extern "C" int pc_bn_finalize(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group,
                              const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                              float* running_var, float* stat, pc_stream s) {
    return pc_bn_finalize_ws(part, nparts_per_group, groups, C, count_per_group, gamma, beta, eps, momentum, running_mean, running_var, stat, nullptr, s);
}

// Finalize + apply in ONE launch (bn_fin_apply_kernel): for layers with at most FA_MAX_NPG partial rows per batch group.  Same results as
// pc_bn_finalize followed by pc_bn_apply (the per-channel sums are taken in double in another, equally fixed order).
constexpr int FA_MAX_NPG = 256;
static int fa_rows_per_block(int64_t rpg, int cblocks, int groups) {
    // about 2048 blocks, at least 128 rows each (the partial rows a block re-reads must stay a fraction of the rows it streams), whole 16-row passes
    int64_t rb = (rpg * cblocks * groups + 2047) / 2048;
    if (rb < 128) rb = 128;
    return (int)((rb + 15) / 16 * 16);
}
extern "C" int pc_bn_finalize_apply_ok(int nparts_per_group, int C) { return nparts_per_group >= 1 && nparts_per_group <= FA_MAX_NPG && C % 4 == 0 ? 1 : 0; }

extern "C" int pc_bn_finalize_apply(const float* part, int nparts_per_group, int groups, int C, int64_t count_per_group, const float* gamma, const float* beta,
                                    float eps, float momentum, float* running_mean, float* running_var, float* stat, const float* z, int ldz, int64_t rows,
                                    float* y, int ldy, int relu, pc_stream s) {
    PC_CHECK_ARG(part && gamma && beta && stat && z && y && groups >= 1 && C > 0 && C % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && rows % groups == 0,
                 "pc_bn_finalize_apply: bad args (C=%d)", C);
    PC_CHECK_ARG(pc_bn_finalize_apply_ok(nparts_per_group, C), "pc_bn_finalize_apply: %d partial rows per group (at most %d: use pc_bn_finalize + pc_bn_apply)",
                 nparts_per_group, FA_MAX_NPG);
    PC_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "pc_bn_finalize_apply: running_mean / running_var go together");
    const int64_t rpg = rows / groups;
    PC_CHECK_ARG(rows * (int64_t)(C / 4) < (1ll << 31) && rpg < (1ll << 31), "elementwise kernels index with 32 bits");
    const int cblocks = cdiv(C, FA_CB), rpb = fa_rows_per_block(rpg, cblocks, groups);
    hipLaunchKernelGGL(bn_fin_apply_kernel, dim3((unsigned)cdiv(rpg, rpb), cblocks, groups), dim3(256), 0, (hipStream_t)s, part, nparts_per_group, groups, C,
                       (double)count_per_group, gamma, beta, eps, momentum, running_mean, running_var, stat, z, ldz, y, ldy, relu, (int)rpg, rpb);
    PC_CHECK_LAUNCH("bn_fin_apply");
    return PC_OK;
}

extern "C" int pc_bn_eval_stat(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float eps, int C, float* stat, pc_stream s) {
    PC_CHECK_ARG(gamma && beta && running_mean && running_var && stat, "pc_bn_eval_stat: null");
    hipLaunchKernelGGL(bn_eval_stat_kernel, dim3(cdiv(C, 256)), dim3(256), 0, (hipStream_t)s, gamma, beta, running_mean, running_var, eps, C, stat);
    PC_CHECK_LAUNCH("bn_eval_stat");
    return PC_OK;
}

extern "C" int pc_bn_apply(const float* z, int ldz, const float* stat, int C, int64_t rows, int groups, float* y, int ldy,
                           int relu, pc_stream s) {
    PC_CHECK_ARG(z && stat && y && C % 4 == 0 && ldz % 4 == 0 && ldy % 4 == 0 && groups >= 1 && rows % groups == 0, "pc_bn_apply: bad args (C=%d)", C);
    const int64_t total4 = rows * (C / 4);
    PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(total4, 2)), dim3(256), 0, (hipStream_t)s, z, ldz, stat, C / 4, total4, rows / groups, y, ldy, relu);
    PC_CHECK_LAUNCH("bn_apply");
    return PC_OK;
}

extern "C" int64_t pc_bn_bwd_ws_floats(int64_t rows, int C, int groups) {
    const int64_t rpg = rows / groups;
    const int64_t npg = (rpg + red_rows_per_block(rpg) - 1) / red_rows_per_block(rpg);
    return (npg * groups * 2 + groups * 2) * (int64_t)C + 64;
}

extern "C" int pc_bn_bwd(const float* dy, int lddy, const float* z, int ldz, const float* stat, int C, int64_t rows, int groups,
                         int relu_flags, float* dz, int lddz, float* dgamma, float* dbeta, int accum, float* ws, pc_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    PC_CHECK_ARG(dy && z && stat && dz && ws && C % 4 == 0 && C <= 1024 && lddy % 4 == 0 && ldz % 4 == 0 && lddz % 4 == 0 &&
                 groups >= 1 && rows % groups == 0, "pc_bn_bwd: bad args (C=%d)", C);
    const int64_t rpg = rows / groups;
    // PICONS_BN_FUSED=1 (read per call: a test switch): layers of at most 16 384 rows per group (the 28 x 28 layers) take at most 192 partial rows
    // per group and the finalize folded into the apply kernel (bn_bwd_fin_apply_kernel) -- two launches instead of three on the dependency chain.
    // Built for VERDICT r4 #4b and measured (profiles/r05_switch_ab.txt): the step does not move (19.25 against 19.25 ms) and the family's
    // single-stream time goes UP (1.43 -> 1.54 ms: every block of the apply kernel repeats the reduction over the partial rows), so it is OFF.
    const bool fused = (relu_flags & 2) && rpg <= 16384;          // asked for by the caller (bit 1 of `relu`): the planner's decision, not an environment read per call
    const int relu = relu_flags & 1;
    int64_t rpb = red_rows_per_block(rpg);
    if (fused && (rpg + 191) / 192 > rpb) rpb = (rpg + 191) / 192;
    const int npg = (int)((rpg + rpb - 1) / rpb);
    float* part = ws;
    float* coef = ws + (size_t)npg * groups * 2 * C;
    {   // blockIdx.y = group keeps block row ranges inside the group
        RedP p;
        p.a = dy; p.lda = lddy; p.b = z; p.ldb = ldz;
        p.stat = stat; p.C4 = C / 4; p.rows = rpg; p.rows_per_group = rpg; p.rows_per_block = rpb;
        p.act = relu ? PC_ACT_RELU : PC_ACT_NONE; p.part = part;
        p.a_gs = rpg * lddy; p.b_gs = rpg * ldz; p.stat_gs = 4 * C; p.part_gs = (int64_t)npg * 2 * C;
        hipLaunchKernelGGL(colreduce_kernel, dim3(npg, groups), dim3(256), 0, s, p);
    }
    PC_CHECK_LAUNCH("bn_bwd reduce");
    if (fused) {
        PC_CHECK_ARG(rows * (int64_t)(C / 4) < (1ll << 31), "elementwise kernels index with 32 bits");
        const int cblocks = cdiv(C, FA_CB), rb2 = fa_rows_per_block(rpg, cblocks, groups);
        hipLaunchKernelGGL(bn_bwd_fin_apply_kernel, dim3((unsigned)cdiv(rpg, rb2), cblocks, groups), dim3(256), 0, s, part, npg, groups, C, (double)rpg, dy, lddy, z, ldz,
                           stat, relu, dz, lddz, dgamma, dbeta, accum, (int)rpg, rb2);
        PC_CHECK_LAUNCH("bn_bwd fin_apply");
        return PC_OK;
    }
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, FIN_CL)), dim3(FIN_T), 0, s, part, npg, groups, C, (double)rpg, coef, dgamma, dbeta, accum);
    const int64_t total4 = rows * (C / 4);
    PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(grid_for(total4, 2)), dim3(256), 0, s, dy, lddy, z, ldz, stat, coef, C / 4, total4, rpg, relu, dz, lddz);
    PC_CHECK_LAUNCH("bn_bwd apply");
    return PC_OK;
}

extern "C" int pc_maxpool_fwd(const pc_pool_desc* d, const float* x, float* y, uint8_t* argmax, pc_stream s) {
    PC_CHECK_ARG(d && x && y && argmax && d->C % 4 == 0 && d->ldi % 4 == 0 && d->ldo % 4 == 0, "pc_maxpool_fwd: bad args");
    PC_CHECK_ARG(d->k[0] * d->k[1] * d->k[2] < 255, "pc_maxpool_fwd: window too large");
    const int64_t npos = (int64_t)d->N * d->To * d->Ho * d->Wo, total4 = npos * (d->C / 4);
    PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    const int nblk = pool_blocks(total4);
    const unsigned ppb = (unsigned)cdiv(npos, nblk);
#define PC_POOL_FWD(...) hipLaunchKernelGGL((maxpool_fwd_kernel<__VA_ARGS__>), dim3(nblk), dim3(256), 0, (hipStream_t)s, *d, x, y, argmax, (unsigned)npos, ppb)
#define PC_POOL_FWD_TILE(ST)                                                                                                                     \
    do {                                                                                                                                         \
        const int64_t items = (int64_t)d->N * d->To * ((d->Ho + 1) / 2) * ((d->Wo + 1) / 2) * (d->C / 4);                                       \
        hipLaunchKernelGGL((maxpool333_fwd_tile_kernel<ST>), dim3(items > 256 ? (unsigned)cdiv(items, 256) : 1), dim3(256), 0, (hipStream_t)s, \
                           *d, x, y, argmax, (unsigned)items);                                                                                   \
    } while (0)
    const bool tile = pool_in_4g(d);
    switch (pool_form(d)) {
        case 1: PC_POOL_FWD(1, 3, 3, 1, 2, 2); break;
        case 2: if (tile) PC_POOL_FWD_TILE(2); else PC_POOL_FWD(3, 3, 3, 2, 1, 1); break;
        case 3: if (tile) PC_POOL_FWD_TILE(1); else PC_POOL_FWD(3, 3, 3, 1, 1, 1); break;
        default: PC_POOL_FWD(0, 0, 0, 0, 0, 0);
    }
#undef PC_POOL_FWD_TILE
#undef PC_POOL_FWD
    PC_CHECK_LAUNCH("maxpool_fwd");
    return PC_OK;
}

extern "C" int pc_maxpool_bwd(const pc_pool_desc* d, const float* dy, const uint8_t* argmax, float* dx, int accum, pc_stream s) {
    PC_CHECK_ARG(d && dy && dx && argmax && d->C % 4 == 0 && d->ldi % 4 == 0 && d->ldo % 4 == 0, "pc_maxpool_bwd: bad args");
    const int64_t npos = (int64_t)d->N * d->Ti * d->Hi * d->Wi, total4 = npos * (d->C / 4);
    PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    const int nblk = pool_blocks(total4);
    const unsigned ppb = (unsigned)cdiv(npos, nblk);
#define PC_POOL_BWD(...) hipLaunchKernelGGL((maxpool_bwd_kernel<__VA_ARGS__>), dim3(nblk), dim3(256), 0, (hipStream_t)s, *d, dy, argmax, dx, accum, (unsigned)npos, ppb)
#define PC_POOL_BWD_TILE(ST)                                                                                                                     \
    do {                                                                                                                                         \
        const int64_t items = pool_tile_items((int64_t)d->N * d->Ti * d->Hi, d->Wi, d->C / 4);                                                  \
        hipLaunchKernelGGL((maxpool333_bwd_tile_kernel<ST, POOL_WT>), dim3(items > 256 ? (unsigned)cdiv(items, 256) : 1), dim3(256), 0, (hipStream_t)s, \
                           *d, dy, argmax, dx, accum, (unsigned)items);                                                                          \
    } while (0)
    switch (pool_form(d)) {
        case 1: PC_POOL_BWD(1, 3, 3, 1, 2, 2); break;
        case 2: PC_POOL_BWD_TILE(2); break;
        case 3: PC_POOL_BWD_TILE(1); break;
        default: PC_POOL_BWD(0, 0, 0, 0, 0, 0);
    }
#undef PC_POOL_BWD_TILE
#undef PC_POOL_BWD
    PC_CHECK_LAUNCH("maxpool_bwd");
    return PC_OK;
}

extern "C" int pc_channel_scale(const float* x, int ldx, const float* scale, int N, int64_t pos_per_n, int C, float* y, int ldy,
                                int accum, pc_stream s) {
    PC_CHECK_ARG(x && scale && y && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0, "pc_channel_scale: bad args");
    const int64_t total4 = (int64_t)N * pos_per_n * (C / 4);
    PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    hipLaunchKernelGGL(chscale_kernel, dim3(grid_for(total4, 2)), dim3(256), 0, (hipStream_t)s, x, ldx, scale, pos_per_n, C / 4, total4, y, ldy, accum);
    PC_CHECK_LAUNCH("channel_scale");
    return PC_OK;
}

extern "C" int64_t pc_act_bwd_ws_floats(int64_t rows, int C) {
    const int64_t rpb = red_rows_per_block(rows);
    return ((rows + rpb - 1) / rpb) * 2 * (int64_t)C + 64;
}

extern "C" int pc_act_bwd(const float* dy, int lddy, const float* y, int ldy, int act, int C, int64_t rows, float* dz, int lddz,
                          float* dbias, int accum, float* ws, pc_stream s_) {
    hipStream_t s = (hipStream_t)s_;
    PC_CHECK_ARG(dy && y && C % 4 == 0 && C <= 1024 && lddy % 4 == 0 && ldy % 4 == 0, "pc_act_bwd: bad args (C=%d)", C);
    const bool write = dz && (act != PC_ACT_NONE || dz != dy);
    const int64_t total4 = rows * (C / 4);
    if (write) {
        PC_CHECK_ARG(lddz % 4 == 0, "pc_act_bwd: lddz");
        PC_CHECK_ARG(total4 < (1ll << 31), "elementwise kernels index with 32 bits: %lld float4 elements", (long long)total4);
    }
    if (dbias) {        // one pass over (dy, y): the partial sums and, where asked for, dz
        PC_CHECK_ARG(ws, "pc_act_bwd: ws required for dbias");
        const int64_t rpb = red_rows_per_block(rows);
        const int nblk = (int)((rows + rpb - 1) / rpb);
        if (write) hipLaunchKernelGGL(act_bwd_reduce_kernel<true>, dim3(nblk), dim3(256), 0, s, dy, lddy, y, ldy, act, C / 4, rows, rpb, dz, lddz, ws);
        else hipLaunchKernelGGL(act_bwd_reduce_kernel<false>, dim3(nblk), dim3(256), 0, s, dy, lddy, y, ldy, act, C / 4, rows, rpb, (float*)nullptr, 0, ws);
        hipLaunchKernelGGL(colsum_finalize_kernel, dim3(cdiv(C, FIN_CL)), dim3(FIN_T), 0, s, ws, nblk, C, dbias, accum);
    } else if (write) {
        hipLaunchKernelGGL(act_bwd_apply_kernel, dim3(grid_for(total4, 2)), dim3(256), 0, s, dy, lddy, y, ldy, act, C / 4, total4, dz, lddz);
    }
    PC_CHECK_LAUNCH("act_bwd");
    return PC_OK;
}

extern "C" int pc_ncdhw_to_ndhwc(const void* src, int src_is_f64, int N, int C, int64_t thw, int W, int Cpad, int flipw, float* dst, pc_stream s) {
    PC_CHECK_ARG(src && dst && Cpad >= C && W > 0 && thw % W == 0, "pc_ncdhw_to_ndhwc: bad args");
    const int64_t total = (int64_t)N * thw;
    if (src_is_f64) hipLaunchKernelGGL(to_ndhwc_kernel<double>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, (const double*)src, N, C, thw, W, Cpad, flipw, dst);
    else hipLaunchKernelGGL(to_ndhwc_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, (const float*)src, N, C, thw, W, Cpad, flipw, dst);
    PC_CHECK_LAUNCH("to_ndhwc");
    return PC_OK;
}

extern "C" int pc_ndhwc_to_ncdhw(const float* src, int ld, int N, int C, int64_t thw, float* dst, pc_stream s) {
    PC_CHECK_ARG(src && dst, "pc_ndhwc_to_ncdhw: null");
    hipLaunchKernelGGL(to_ncdhw_kernel, dim3(grid_for((int64_t)N * C * thw)), dim3(256), 0, (hipStream_t)s, src, ld, N, C, thw, dst);
    PC_CHECK_LAUNCH("to_ncdhw");
    return PC_OK;
}

extern "C" int pc_transpose_batched(const float* src, int batch, int R, int Cc, int64_t src_batch_stride, int src_ld, float* dst,
                                    int64_t dst_batch_stride, int dst_ld, int accum, pc_stream s) {
    PC_CHECK_ARG(src && dst && batch >= 1 && batch <= 65535 && R >= 1 && Cc >= 1, "pc_transpose_batched: bad args");
    PC_CHECK_ARG(cdiv(R, 32) <= 65535, "pc_transpose_batched: too many row tiles");
    hipLaunchKernelGGL(transpose_kernel, dim3(cdiv(Cc, 32), cdiv(R, 32), batch), dim3(256), 0, (hipStream_t)s, src, R, Cc, src_batch_stride,
                       src_ld, dst, dst_batch_stride, dst_ld, accum);
    PC_CHECK_LAUNCH("transpose");
    return PC_OK;
}

extern "C" int pc_transpose_multi(const pc_transpose_job* jobs, int njobs, pc_stream s) {
    PC_CHECK_ARG(jobs && njobs >= 1, "pc_transpose_multi: bad args");
    for (int j = 0; j < njobs; ++j) {
        const pc_transpose_job& a = jobs[j];
        PC_CHECK_ARG(a.src && a.dst && a.batch >= 1 && a.R >= 1 && a.C >= 1, "pc_transpose_multi: bad job %d", j);
        PC_CHECK_ARG(a.nslices >= 0 && (a.nslices <= 1 || a.slice_stride > 0), "pc_transpose_multi: job %d has %d slices %lld floats apart", j, a.nslices, (long long)a.slice_stride);
        PC_CHECK_ARG(a.nslices <= 1 || (a.C <= a.src_ld && a.src_ld % 4 == 0 && a.slice_stride % 4 == 0 && a.src_batch_stride % 4 == 0 && a.src % 16 == 0),
                     "pc_transpose_multi: job %d sums slice images: src_ld (>= C) and the strides must be multiples of 4 floats and src 16-byte aligned", j);
    }
    // Jobs by class (the jobs of a call are independent, so their order is free): rows -- R == 1, or C == 1 read with unit stride and
    // without slices -- go to relayout_rows_kernel, everything else to the tile kernel.  Both take their jobs by value, TM_JOBS to a launch.
    const auto is_rows = [](const pc_transpose_job& a) { return a.R == 1 || (a.C == 1 && a.src_ld == 1 && a.nslices <= 1); };
    TPack pk;
    pk.n = 0;
    int tiles = 0;
    const auto flush_tiles = [&]() -> int {
        if (!pk.n) return PC_OK;
        pk.first[pk.n] = tiles;
        hipLaunchKernelGGL(transpose_multi_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)s, pk);
        PC_CHECK_LAUNCH("transpose_multi");
        pk.n = 0; tiles = 0;
        return PC_OK;
    };
    for (int j = 0; j < njobs; ++j) {
        const pc_transpose_job& a = jobs[j];
        if (is_rows(a)) continue;
        TJobK k;
        k.src = (const float*)(uintptr_t)a.src; k.dst = (float*)(uintptr_t)a.dst; k.sbs = a.src_batch_stride; k.dbs = a.dst_batch_stride;
        k.R = a.R; k.Cc = a.C; k.sld = a.src_ld; k.dld = a.dst_ld; k.accum = a.accum; k.nsl = a.nslices; k.sst = a.slice_stride;
        // 32-row tiles (one 16-byte quad per thread and image, 256 threads busy) unless the job is too small to give every CU a block: then
        // 8-row tiles, four times the blocks (the sum over many images is a chain of dependent loads per thread)
        k.tr = (a.nslices > 1 && (long long)a.batch * cdiv(a.C, 32) * cdiv(a.R, 32) < 192) ? 8 : 32; k.pad_ = 0;
        k.tiles_c = cdiv(a.C, 32); k.tiles_rc = k.tiles_c * cdiv(a.R, k.tr);
        const long long t = (long long)a.batch * k.tiles_rc;
        PC_CHECK_ARG(t < (1ll << 30), "pc_transpose_multi: job %d is too large", j);
        if (tiles + t >= (1ll << 30)) { const int rc = flush_tiles(); if (rc != PC_OK) return rc; }
        pk.j[pk.n] = k;
        pk.first[pk.n++] = tiles;
        tiles += (int)t;
        if (pk.n == TM_JOBS) { const int rc = flush_tiles(); if (rc != PC_OK) return rc; }
    }
    { const int rc = flush_tiles(); if (rc != PC_OK) return rc; }
    RPack rp;
    rp.n = 0;
    int units = 0;
    const auto flush_rows = [&]() -> int {
        if (!rp.n) return PC_OK;
        rp.first[rp.n] = units;
        hipLaunchKernelGGL(relayout_rows_kernel, dim3(units), dim3(256), 0, (hipStream_t)s, rp);
        PC_CHECK_LAUNCH("transpose_multi rows");
        rp.n = 0; units = 0;
        return PC_OK;
    };
    for (int j = 0; j < njobs; ++j) {
        const pc_transpose_job& a = jobs[j];
        if (!is_rows(a)) continue;
        RJobK k;
        k.src = (const float*)(uintptr_t)a.src; k.dst = (float*)(uintptr_t)a.dst; k.sbs = a.src_batch_stride; k.dbs = a.dst_batch_stride; k.sst = a.slice_stride;
        k.batch = a.batch; k.accum = a.accum; k.nsl = a.nslices;
        if (a.R == 1) { k.L = a.C; k.dstep = a.dst_ld; }   // dst[b][c][0] (+)= src[b][0][c]
        else { k.L = a.R; k.dstep = 1; }                   // dst[b][0][r] (+)= src[b][r][0], src_ld = 1
        k.qpr = cdiv(k.L, 4);
        const bool rows_al = a.batch == 1 || (a.src_batch_stride % 4 == 0);
        k.vld = a.nslices > 1 || (a.src % 16 == 0 && rows_al && k.L % 4 == 0);
        k.vst = k.dstep == 1 && a.dst % 16 == 0 && (a.batch == 1 || a.dst_batch_stride % 4 == 0);
        const long long u = ((long long)a.batch * k.qpr + 255) / 256;
        PC_CHECK_ARG(u < (1ll << 30), "pc_transpose_multi: job %d is too large", j);
        if (units + u >= (1ll << 30)) { const int rc = flush_rows(); if (rc != PC_OK) return rc; }
        rp.j[rp.n] = k;
        rp.first[rp.n++] = units;
        units += (int)u;
        if (rp.n == TM_JOBS) { const int rc = flush_rows(); if (rc != PC_OK) return rc; }
    }
    return flush_rows();
}

extern "C" int pc_wgrad_fold_group(void) { return 16; }

extern "C" int pc_wgrad_fold(float* ws, int64_t image_floats, int nslices, pc_stream s) {
    PC_CHECK_ARG(ws && image_floats > 0 && image_floats % 4 == 0 && nslices >= 1 && (uintptr_t)ws % 16 == 0, "pc_wgrad_fold: bad args (image %lld floats, %d slices)", (long long)image_floats, nslices);
    constexpr int GROUP = 16;
    if (nslices <= 1) return PC_OK;
    const int64_t total = (image_floats / 4) * cdiv(nslices, GROUP);
    hipLaunchKernelGGL(slices_fold_kernel<GROUP>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, ws, image_floats / 4, nslices, total);
    PC_CHECK_LAUNCH("slices_fold");
    return PC_OK;
}

extern "C" int pc_col2im(const float* cols, int N, int Ho, int Wo, int KH, int KW, int C, float* dx, int lddx, int accum, pc_stream s) {
    PC_CHECK_ARG(cols && dx && C % 4 == 0 && lddx % 4 == 0, "pc_col2im: bad args");
    const int64_t total4 = (int64_t)N * (Ho + KH - 1) * (Wo + KW - 1) * (C / 4);
    hipLaunchKernelGGL(col2im_kernel, dim3(grid_for(total4)), dim3(256), 0, (hipStream_t)s, cols, N, Ho, Wo, KH, KW, C / 4, dx, lddx, accum, total4);
    PC_CHECK_LAUNCH("col2im");
    return PC_OK;
}

extern "C" int pc_fill(float* p, int64_t n, float v, pc_stream s) {
    PC_CHECK_ARG(p || n == 0, "pc_fill: null");
    if (n == 0) return PC_OK;
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)s, p, n, v);
    PC_CHECK_LAUNCH("fill");
    return PC_OK;
}

extern "C" int pc_axpy(float* y, const float* x, int64_t n, float a, pc_stream s) {
    PC_CHECK_ARG((y && x) || n == 0, "pc_axpy: null");
    if (n == 0) return PC_OK;
    hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)s, y, x, n, a);
    PC_CHECK_LAUNCH("axpy");
    return PC_OK;
}

extern "C" int pc_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, int step,
                            float gscale, pc_stream s) {
    PC_CHECK_ARG(p && g && m && v && step >= 1 && n >= 0, "pc_adam_step: bad args");
    if (n == 0) return PC_OK;                  // an un-armed early-Adam op of the backward list
    // torch.optim.Adam (main_ucf101.py:416) holds its betas as Python doubles: 1 - beta and the bias corrections 1 - beta^t are computed in
    // double and only then rounded to fp32 (1 - 0.999 -> 0.001f; in fp32, 1.f - 0.999f = 0.00100004673: 4.7e-5 off in every second-moment
    // increment).  The ABI carries floats, so the double the caller meant is recovered as the shortest decimal that round-trips the float.
    const double b1d = pc_decimal_of_float(b1), b2d = pc_decimal_of_float(b2);
    const double bc1 = 1.0 - pow(b1d, step), bc2 = 1.0 - pow(b2d, step);
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 4)), dim3(256), 0, (hipStream_t)s, p, g, m, v, n, (float)(lr / bc1), b1, b2,
                       (float)(1.0 - b1d), (float)(1.0 - b2d), eps, (float)(1.0 / sqrt(bc2)), gscale);
    PC_CHECK_LAUNCH("adam");
    return PC_OK;
}
