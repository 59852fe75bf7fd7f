// The probability map of a pass against a truth map at every mask threshold at once (detect.DetectEngine.sweep): per frame the pixels counted
// by (truth or not, how many of N ascending threshold words are <= the pixel's probability word).  The pixels positive at threshold k are
// those with more than k words at or below them, so (inter, union, gt) at every threshold are suffix sums of one frame's 2 * (N + 1) cells.
//   pc_prob_truth_hist   prob_hist_kernel on a grid of bpf blocks per frame (crosstab.hip's rule: a function of H * W alone, at most 64): each
//                        block leaves the table of its share of the frame's four-pixel groups in `ws`; prob_hist_fold_kernel, one block per
//                        frame, adds the partials in block order and writes cell [0][0] as H * W minus the rest, so the pixel that is common
//                        by far -- no truth, probability below the first threshold -- costs no LDS traffic.
// The walk is crosstab_kernel's with a 16-bit map on the pred side: groups of four pixels, the loads of four groups in flight, truth through
// map_bytes, the four probabilities as one 8-byte load where the frame starts on an 8-byte address (a frame starts at any 2-byte address when
// H * W is odd: element by element then, as in a frame's tail group), a per-thread (cell, count) run flushed into per-wave LDS bins.
// The thresholds travel in the kernel-argument struct, 128 bytes beside the pointers, as the other small tables of the detect kernels do: a
// staged copy would need a device buffer of the library's own, an ordering against the stream, and a host source that outlives it.  Each
// block spreads them into an LDS table padded with a word no probability reaches; a pixel at or above the first threshold -- tested first,
// against a scalar -- finds its count by a branch-free binary search there.
// Integer addition only, no global atomics, nothing waits on another block (the fold is a launch of its own), every output word is a function
// of the input alone.
#include "common.h"
#include "rowbytes.h"
#include "probwords.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
constexpr int MAXN = PC_SWEEP_MAX_THRESHOLDS;
constexpr int MAXCELLS = 2 * (MAXN + 1);
constexpr int TAB = 2 * MAXN;                                        // the search table: the words, then a word above every probability
constexpr int MAX_GRID = 1 << 23;                                    // blocks of one launch: 2^31 threads
static_assert(MAXN == 64 && NW * MAXCELLS * 4 + TAB * 4 == 2592, "static LDS of prob_hist_kernel");

// blocks per frame: ~4 groups of four pixels per thread, at most 64.  A function of H * W alone (cross_bpf of crosstab.hip).
inline int hist_bpf(int64_t HW) {
    const int64_t n = ((HW + 3) / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

struct HistK {
    const uint16_t* prob; const uint8_t* truth;                      // frame 0 of the launch's frames
    int32_t* ws;                                                     // [frame][bpf][cells] of the launch's frames
    int H, W, N, bpf, top;                                           // top: the largest power of two <= N, the search's first step
    uint32_t thr[MAXN / 2];                                          // word 2i in the low half, 2i + 1 in the high half
};

// grid (frames * bpf): block x is share x % bpf of frame x / bpf.  The bpf blocks of a frame stride over its groups of four consecutive
// pixels.  A pixel without truth and below the first threshold is not counted at all (cell [0][0] comes out of the fold), as is a group of
// four such pixels, or one past the frame's end.
__global__ __launch_bounds__(256) void prob_hist_kernel(const HistK p) {
    __shared__ int bins[NW][MAXCELLS];
    __shared__ uint32_t tab[TAB];
    const int tid = threadIdx.x, wv = tid >> 6, N = p.N, side = N + 1, cells = 2 * side, top = p.top;
    const uint32_t thr0 = p.thr[0] & 0xffffu;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W, total4 = (HW + 3u) >> 2;
    const uint32_t fr = blockIdx.x / (uint32_t)p.bpf, part = blockIdx.x % (uint32_t)p.bpf, stride = (uint32_t)p.bpf * BT;
    const uint16_t* __restrict__ pp = p.prob + (size_t)fr * HW;
    const uint8_t* __restrict__ tp = p.truth + (size_t)fr * HW;
    const bool wide = ((uintptr_t)pp & 7) == 0;                      // a group starts 8 * gr bytes into its frame
    for (int w = 0; w < NW; ++w)
        for (int t = tid; t < cells; t += BT) bins[w][t] = 0;
    if (tid < TAB) tab[tid] = tid < N ? (p.thr[tid >> 1] >> (16 * (tid & 1))) & 0xffffu : 0x10000u;
    __syncthreads();

    int cur = -1, cnt = 0;                                           // the cell the thread is in; nothing to flush while cnt == 0
    for (uint32_t g0 = part * BT + tid; g0 < total4; g0 += stride * 4) {
        uint2 va[4];
        uint32_t vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t gr = g0 + u * stride, px = gr << 2;
            const bool in = gr < total4;
            const int n = in ? (int)(HW - px < 4u ? HW - px : 4u) : 0;
            va[u] = prob_words(pp + (in ? px : 0u), n, wide);
            vb[u] = map_bytes(tp + (in ? px : 0u), n);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t lo = va[u].x, hi = va[u].y;
            if (vb[u] == 0u && (lo & 0xffffu) < thr0 && (lo >> 16) < thr0 && (hi & 0xffffu) < thr0 && (hi >> 16) < thr0) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t q = ((e < 2 ? lo : hi) >> (16 * (e & 1))) & 0xffffu;
                const bool t = ((vb[u] >> (8 * e)) & 0xffu) != 0u;
                if (q < thr0 && !t) continue;
                int b = 0;
                if (q >= thr0)
                    for (int s = top; s > 0; s >>= 1)
                        if (tab[b + s - 1] <= q) b += s;                 // b + s - 1 <= 2 * top - 2 < TAB
                const int cell = (t ? side : 0) + b;
                if (cell != cur) {
                    if (cnt) atomicAdd(&bins[wv][cur], cnt);
                    cur = cell; cnt = 0;
                }
                ++cnt;
            }
        }
    }
    if (cnt) atomicAdd(&bins[wv][cur], cnt);
    __syncthreads();
    int32_t* o = p.ws + (size_t)blockIdx.x * (size_t)cells;
    for (int t = tid; t < cells; t += BT) {
        int n = bins[0][t];
#pragma unroll
        for (int w = 1; w < NW; ++w) n += bins[w][t];
        o[t] = n;
    }
}

// grid (frames): the frame's bpf partial tables added in block order into its cells of `out`; cell 0 = H * W - all the others.
__global__ __launch_bounds__(256) void prob_hist_fold_kernel(const int32_t* __restrict__ ws, int32_t* __restrict__ out, int cells, int bpf, uint32_t HW) {
    __shared__ int wsum[NW];
    const int tid = threadIdx.x;
    const int32_t* q = ws + (size_t)blockIdx.x * (size_t)bpf * (size_t)cells;
    int32_t* o = out + (size_t)blockIdx.x * (size_t)cells;
    int rest = 0;
    for (int t = tid; t < cells; t += BT) {
        if (t == 0) continue;
        int n = 0;
        for (int b = 0; b < bpf; ++b) n += q[(size_t)b * cells + t];
        o[t] = n;
        rest += n;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) rest += __shfl_xor(rest, s, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = rest;
    __syncthreads();
    if (tid == 0) {
        int all = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) all += wsum[w];
        o[0] = (int32_t)(HW - (uint32_t)all);
    }
}

}  // namespace

extern "C" int64_t pc_prob_truth_hist_ws_bytes(int nf, int H, int W, int N) {
    if (nf < 1 || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return -1;
    if (N < 1 || N > PC_SWEEP_MAX_THRESHOLDS) return -1;
    return (int64_t)nf * hist_bpf((int64_t)H * W) * (int64_t)(2 * (N + 1)) * 4;
}

extern "C" int pc_prob_truth_hist(const uint16_t* prob, const uint8_t* truth, int F, int H, int W, int f0, int nf, const uint16_t* thr, int N,
                                  int32_t* out, void* ws, pc_stream s) {
    const char* who = "pc_prob_truth_hist";
    PC_CHECK_ARG(prob && truth && thr && out && ws, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG(N >= 1 && N <= PC_SWEEP_MAX_THRESHOLDS, "%s: N = %d outside 1..%d", who, N, PC_SWEEP_MAX_THRESHOLDS);
    PC_CHECK_ARG(thr[0] != 0, "%s: a threshold word of 0 (every pixel is at or above it)", who);
    for (int k = 1; k < N; ++k)
        PC_CHECK_ARG(thr[k] > thr[k - 1], "%s: thresholds not strictly ascending: word %d = %d after %d", who, k, (int)thr[k], (int)thr[k - 1]);
    PC_CHECK_ARG((uintptr_t)prob % 2 == 0, "%s: prob must be 2-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)out % 4 == 0, "%s: out must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)ws % 8 == 0, "%s: ws must be 8-byte aligned", who);
    const size_t HW = (size_t)H * (size_t)W;
    const int cells = 2 * (N + 1), bpf = hist_bpf((int64_t)HW);
    const int per = MAX_GRID / bpf;                                  // frames of one launch (a video is one launch; only a map of millions of frames is cut)
    HistK k;
    k.H = H; k.W = W; k.N = N; k.bpf = bpf;
    for (k.top = 1; k.top * 2 <= N; k.top *= 2) {}
    for (int i = 0; i < MAXN / 2; ++i)
        k.thr[i] = (2 * i < N ? (uint32_t)thr[2 * i] : 0u) | (2 * i + 1 < N ? (uint32_t)thr[2 * i + 1] << 16 : 0u);
    for (int64_t c0 = 0; c0 < nf; c0 += per) {
        const int n = (int)(nf - c0 < per ? nf - c0 : per);
        const size_t fa = (size_t)f0 + (size_t)c0;
        k.prob = prob + fa * HW; k.truth = truth + fa * HW;
        k.ws = (int32_t*)ws + (size_t)c0 * (size_t)bpf * (size_t)cells;
        hipLaunchKernelGGL(prob_hist_kernel, dim3((unsigned)(n * bpf)), dim3(BT), 0, (hipStream_t)s, k);
        PC_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(prob_hist_fold_kernel, dim3((unsigned)n), dim3(BT), 0, (hipStream_t)s, (const int32_t*)k.ws, out + fa * (size_t)cells, cells, bpf,
                           (uint32_t)HW);
        PC_CHECK_LAUNCH(who);
    }
    return PC_OK;
}
