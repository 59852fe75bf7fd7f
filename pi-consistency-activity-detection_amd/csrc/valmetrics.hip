// Validation metrics on the device: everything val_model_interface and the body of validate (main_ucf101.py:33-47, 241-264) compute from one
// batch -- BCEWithLogits + Dice (utils/losses.py:44-57), SpreadLoss (:14-37), the argmax match count of get_accuracy (utils/metrics.py:7-13) and
// the per-clip sums IOU2 takes (:171-193) -- in two launches and one record, instead of a dozen ATen launches, two .item() syncs, a D2H of
// the logits and numpy passes over them.  HBM-bound: every logit and every truth pixel is read once (8 bytes per pixel).
// Arithmetic and order follow loss.hip: per-element terms in fp32, sums in double, block partials in a caller-owned workspace added in block
// order by the final stage -- no atomics on floating-point data, so a record is bit-identical from run to run.
#include "common.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
enum { V_BCE, V_SY, V_S, V_Y, V_ND };         // double partials per block: sum bce terms, sum s*y, sum s, sum y
enum { V_INTER, V_UNION, V_GT, V_NI = 4 };    // int32 partials per block (padded to 4)
constexpr int REC_HEAD = 10;                  // record: 8 float scalars, n_correct, B, then [B][3] counts

// blocks per clip: ~4 float4 per thread, at most 256 (the grid-stride loop covers the rest)
inline int val_nbx(int64_t pix4) {
    int64_t n = (pix4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 256 ? 256 : n));
}

struct ValK {
    const float* x; const float* y; const float* pred; const int32_t* action;
    int B, C, nbx; int64_t pix4;
    double* dpart;       // [B][nbx][V_ND]
    double* clipd;       // [B][V_ND]
    int32_t* ipart;      // [B][nbx][V_NI]
    int32_t* rec;
};

inline void carve(ValK& k, float* ws) {
    double* w = (double*)ws;
    k.dpart = w; w += (size_t)k.B * k.nbx * V_ND;
    k.clipd = w; w += (size_t)k.B * V_ND;
    k.ipart = (int32_t*)w;
}

// ---- stage 1: grid (blocks per clip, B), as loss_pass1.  One wave-level reduction per quantity, one block barrier for all seven.
__global__ __launch_bounds__(256) void val_pass1(const ValK p) {
    __shared__ double shd[NW][V_ND];
    __shared__ int shi[NW][V_NI];
    const int b = blockIdx.y;
    const f32x4* xp = (const f32x4*)p.x + (size_t)b * p.pix4;
    const f32x4* yp = (const f32x4*)p.y + (size_t)b * p.pix4;
    double q[V_ND] = {0.0, 0.0, 0.0, 0.0};
    int inter = 0, uni = 0, gnz = 0;
    for (int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x; i < p.pix4; i += (int64_t)p.nbx * BT) {
        const f32x4 xv = xp[i], yv = yp[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = xv[e], y = yv[e];
            // one exponential serves both terms: exp(-|x|) is BCEWithLogits' argument, and sigmoid(x) = 1 / (1 + exp(-x)) for x >= 0,
            // exp(x) / (1 + exp(x)) below (the same value without the overflow of exp(-x))
            const float en = expf(-fabsf(x));
            const float s = x >= 0.f ? 1.0f / (1.0f + en) : en / (1.0f + en);
            q[V_BCE] += (double)(fmaxf(x, 0.f) - x * y + log1pf(en));
            q[V_SY] += (double)(s * y); q[V_S] += (double)s; q[V_Y] += (double)y;
            // validate's `maskout_np > 0` (strict: 0.0 and -0.0 are background) against binary truth
            const bool on = x > 0.f, t = y != 0.f;
            inter += on && t; uni += on || t; gnz += t;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < V_ND; ++k) {
        const double v = wave_sum_d(q[k]);
        if (lane == 0) shd[wv][k] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inter += __shfl_xor(inter, o, 64); uni += __shfl_xor(uni, o, 64); gnz += __shfl_xor(gnz, o, 64);
    }
    if (lane == 0) { shi[wv][V_INTER] = inter; shi[wv][V_UNION] = uni; shi[wv][V_GT] = gnz; }
    __syncthreads();
    const size_t blk = (size_t)b * p.nbx + blockIdx.x;
    if (threadIdx.x < V_ND) {
        const int k = threadIdx.x;
        double v = shd[0][k];
        for (int w = 1; w < NW; ++w) v += shd[w][k];
        p.dpart[blk * V_ND + k] = v;
    } else if (threadIdx.x < V_ND + 3) {
        const int k = threadIdx.x - V_ND;
        int v = shi[0][k];
        for (int w = 1; w < NW; ++w) v += shi[w][k];
        p.ipart[blk * V_NI + k] = v;
    }
}

// ---- final stage (one block): the clips' sums in block order, the batch's in clip order, SpreadLoss, the argmax match count, the record.
__global__ __launch_bounds__(256) void val_final(const ValK p, double npix) {
    __shared__ double shl[NW], sha[NW];
    __shared__ int ncorr, bad;
    const int tid = threadIdx.x;
    if (tid == 0) { ncorr = 0; bad = 0; }
    for (int idx = tid; idx < p.B * 7; idx += BT) {
        const int b = idx / 7, k = idx - b * 7;
        if (k < V_ND) {
            const double* src = p.dpart + (size_t)b * p.nbx * V_ND + k;
            double v = 0.0;
            for (int x = 0; x < p.nbx; ++x) v += src[(size_t)x * V_ND];
            p.clipd[b * V_ND + k] = v;
        } else {
            const int32_t* src = p.ipart + (size_t)b * p.nbx * V_NI + (k - V_ND);
            int v = 0;
            for (int x = 0; x < p.nbx; ++x) v += src[(size_t)x * V_NI];
            p.rec[REC_HEAD + b * 3 + (k - V_ND)] = v;
        }
    }
    __syncthreads();
    // SpreadLoss (utils/losses.py:14-37, r = 0: margin 0.2) over all B rows; a row whose action is outside [0, C) makes the class losses NaN
    double l = 0.0, al = 0.0;
    const int BC = p.B * p.C;
    for (int e = tid; e < BC; e += BT) {
        const int i = e / p.C, a = p.action[i];
        if ((unsigned)a >= (unsigned)p.C) continue;
        const float d = p.pred[(size_t)i * p.C + a] - p.pred[e];
        const float v = 0.2f - d, va = 0.9f - d;
        if (v > 0.f) l += (double)(v * v);
        if (va > 0.f) al += (double)(va * va);
    }
    // get_accuracy: torch.max keeps the first maximum
    for (int i = tid; i < p.B; i += BT) {
        const int a = p.action[i];
        if ((unsigned)a >= (unsigned)p.C) { atomicOr(&bad, 1); continue; }
        const float* row = p.pred + (size_t)i * p.C;
        int best = 0;
        float bv = row[0];
        for (int c = 1; c < p.C; ++c) if (row[c] > bv) { bv = row[c]; best = c; }
        if (best == a) atomicAdd(&ncorr, 1);
    }
    l = wave_sum_d(l); al = wave_sum_d(al);
    if ((tid & 63) == 0) { shl[tid >> 6] = l; sha[tid >> 6] = al; }
    __syncthreads();
    if (tid != 0) return;
    double g[V_ND] = {0.0, 0.0, 0.0, 0.0};
    double iou = 0.0;
    int nvalid = 0;
    for (int b = 0; b < p.B; ++b) {
        for (int k = 0; k < V_ND; ++k) g[k] += p.clipd[b * V_ND + k];
        const int* c = p.rec + REC_HEAD + b * 3;
        if (c[V_GT] > 0) { iou += (double)c[V_INTER] / (double)c[V_UNION]; ++nvalid; }       // IOU2 is NaN for an empty truth: validate leaves the clip out
    }
    const double L = ((shl[0] + shl[1]) + shl[2]) + shl[3], A = ((sha[0] + sha[1]) + sha[2]) + sha[3];
    const double nb = (double)p.B;
    const double bce = g[V_BCE] / (nb * npix);
    const double dice = 1.0 - (2.0 * g[V_SY] + 1.0) / (g[V_S] + g[V_Y] + 1.0);
    double cls = (L / nb - 0.2 * 0.2) / nb;          // divides by b twice (:34-35)
    double acls = A / nb - 0.9 * 0.9;
    if (bad) cls = acls = __longlong_as_double(0x7ff8000000000000ll);
    const double loc = bce + dice;
    float* f = (float*)p.rec;
    f[0] = (float)(loc + cls); f[1] = (float)loc; f[2] = (float)cls; f[3] = (float)acls; f[4] = (float)bce; f[5] = (float)dice;
    f[6] = (float)iou; f[7] = (float)nvalid;
    p.rec[8] = ncorr; p.rec[9] = p.B;
}

inline bool val_shape_ok(int B, int64_t pix) { return B >= 1 && B <= 65535 && pix >= 4 && pix % 4 == 0 && pix < (1ll << 31); }

}  // namespace

extern "C" int pc_val_record_words(int B) { return B >= 1 && B <= 65535 ? REC_HEAD + 3 * B : -1; }

extern "C" int64_t pc_val_metrics_ws_floats(int B, int64_t pix) {
    if (!val_shape_ok(B, pix)) return -1;
    const int64_t nbx = val_nbx(pix / 4);
    return 2 * ((int64_t)B * nbx * V_ND + (int64_t)B * V_ND) + (int64_t)B * nbx * V_NI;
}

extern "C" int pc_val_metrics(const float* output, const float* loc_msk, const float* predicted_action, const int32_t* action, int B, int64_t pix,
                              int C, int32_t* record, float* ws, pc_stream s_) {
    PC_CHECK_ARG(output && loc_msk && predicted_action && action && record && ws, "pc_val_metrics: null pointer");
    PC_CHECK_ARG(B >= 1 && B <= 65535, "pc_val_metrics: B = %d outside [1, 65535]", B);
    PC_CHECK_ARG(C >= 1 && (int64_t)B * C < (1ll << 31), "pc_val_metrics: C = %d (B = %d)", C, B);
    PC_CHECK_ARG(val_shape_ok(B, pix), "pc_val_metrics: pix = %lld must be a positive multiple of 4 below 2^31", (long long)pix);
    PC_CHECK_ARG(((uintptr_t)output % 16 == 0) && ((uintptr_t)loc_msk % 16 == 0) && ((uintptr_t)ws % 16 == 0), "pc_val_metrics: 16-byte alignment of output / loc_msk / ws");
    PC_CHECK_ARG(((uintptr_t)predicted_action % 4 == 0) && ((uintptr_t)action % 4 == 0) && ((uintptr_t)record % 4 == 0), "pc_val_metrics: 4-byte alignment of predicted_action / action / record");
    hipStream_t s = (hipStream_t)s_;
    ValK k;
    k.x = output; k.y = loc_msk; k.pred = predicted_action; k.action = action;
    k.B = B; k.C = C; k.pix4 = pix / 4; k.nbx = val_nbx(k.pix4);
    k.rec = record;
    carve(k, ws);
    hipLaunchKernelGGL(val_pass1, dim3(k.nbx, B), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(val_final, dim3(1), dim3(BT), 0, s, k, (double)pix);
    PC_CHECK_LAUNCH("val_metrics");
    return PC_OK;
}
