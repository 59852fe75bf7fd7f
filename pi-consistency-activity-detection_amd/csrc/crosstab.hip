// A map of a pass against a truth map (detect.DetectEngine.score): the pixels of every frame cross-tabulated by (pred slot, truth slot), what
// f-mAP / v-mAP and a per-instance IoU against truth actors are made of, and what a caller had to copy every mask to the host for.
//   pc_map_crosstab   crosstab_kernel on a grid of bpf blocks per frame (a function of H * W alone, at most 64, as pc_detect_frames_views has
//                     it): each block leaves the table of its share of the frame's four-pixel groups in `ws`; crosstab_fold_kernel, one block
//                     per frame, adds the partials in block order and writes the background / background cell as H * W minus the rest, so the
//                     pixel that is common by far costs no LDS traffic.
// The walk is instance_overlaps_kernel's (instances.hip) with a second map in place of a later frame: groups of four pixels through map_bytes
// on each side, the loads of four groups in flight, a per-thread count of the pair it is in flushed into per-wave LDS bins.  Unlike there the
// truth is read everywhere: truth under predicted background is what union and gt are made of.
// Integer addition only, no global atomics, nothing waits on another block (the fold is a launch of its own), every output word is a function
// of the input alone.
#include "common.h"
#include "rowbytes.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
constexpr int MAXSIDE = PC_CROSS_MAX_SLOTS + 2;                       // background, 1..32, other foreground
constexpr int MAXCELLS = MAXSIDE * MAXSIDE;
constexpr int MAX_GRID = 1 << 23;                                    // blocks of one launch: 2^31 threads
static_assert(NW * MAXCELLS * 4 == 18496, "static LDS of crosstab_kernel");

// blocks per frame: ~4 groups of four pixels per thread, at most 64.  A function of H * W alone (det_views_bpf of detect.hip).
inline int cross_bpf(int64_t HW) {
    const int64_t n = ((HW + 3) / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

struct CrossK {
    const uint8_t* pred; const uint8_t* truth;                       // frame 0 of the launch's frames
    int32_t* ws;                                                     // [frame][bpf][cells] of the launch's frames
    int H, W, P, A, bpf;
};

// grid (frames * bpf): block x is share x % bpf of frame x / bpf.  The bpf blocks of a frame stride over its groups of four consecutive
// pixels; pred and truth are two allocations, and a frame starts H * W bytes into each, so for odd H * W the two sides sit differently in
// their dwords: each goes through map_bytes on its own.  A group whose two dwords are zero is background on background and is not counted
// at all (cell [0][0] comes out of the fold), as is such a pixel inside a group.
__global__ __launch_bounds__(256) void crosstab_kernel(const CrossK p) {
    __shared__ int bins[NW][MAXCELLS];
    const int tid = threadIdx.x, wv = tid >> 6, P = p.P, A = p.A, SA = A + 2, cells = (P + 2) * SA;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W, total4 = (HW + 3u) >> 2;
    const uint32_t fr = blockIdx.x / (uint32_t)p.bpf, part = blockIdx.x % (uint32_t)p.bpf, stride = (uint32_t)p.bpf * BT;
    const uint8_t* __restrict__ pp = p.pred + (size_t)fr * HW;
    const uint8_t* __restrict__ tp = p.truth + (size_t)fr * HW;
    for (int w = 0; w < NW; ++w)
        for (int t = tid; t < cells; t += BT) bins[w][t] = 0;
    __syncthreads();

    int cur = -1, cnt = 0;                                           // the pair the thread is in; nothing to flush while cnt == 0
    for (uint32_t g0 = part * BT + tid; g0 < total4; g0 += stride * 4) {
        uint32_t va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t gr = g0 + u * stride, px = gr << 2;
            const bool in = gr < total4;
            const int n = in ? (int)(HW - px < 4u ? HW - px : 4u) : 0;
            va[u] = map_bytes(pp + (in ? px : 0u), n);
            vb[u] = map_bytes(tp + (in ? px : 0u), n);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((va[u] | vb[u]) == 0u) continue;                     // background on background (or a group past the frame's end)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = (int)((va[u] >> (8 * e)) & 0xffu), b = (int)((vb[u] >> (8 * e)) & 0xffu);
                if ((a | b) == 0) continue;
                const int pair = (a <= P ? a : P + 1) * SA + (b <= A ? b : A + 1);
                if (pair != cur) {
                    if (cnt) atomicAdd(&bins[wv][cur], cnt);
                    cur = pair; cnt = 0;
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
__global__ __launch_bounds__(256) void crosstab_fold_kernel(const int32_t* __restrict__ ws, int32_t* __restrict__ out, int cells, int bpf, uint32_t HW) {
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

extern "C" int64_t pc_map_crosstab_ws_bytes(int nf, int H, int W, int P, int A) {
    if (nf < 1 || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return -1;
    if (P < 1 || P > PC_CROSS_MAX_SLOTS || A < 1 || A > PC_CROSS_MAX_SLOTS) return -1;
    return (int64_t)nf * cross_bpf((int64_t)H * W) * (int64_t)((P + 2) * (A + 2)) * 4;
}

extern "C" int pc_map_crosstab(const uint8_t* pred, const uint8_t* truth, int F, int H, int W, int f0, int nf, int P, int A, int32_t* out, void* ws,
                               pc_stream s) {
    const char* who = "pc_map_crosstab";
    PC_CHECK_ARG(pred && truth && out && ws, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG(P >= 1 && P <= PC_CROSS_MAX_SLOTS, "%s: P = %d outside 1..%d", who, P, PC_CROSS_MAX_SLOTS);
    PC_CHECK_ARG(A >= 1 && A <= PC_CROSS_MAX_SLOTS, "%s: A = %d outside 1..%d", who, A, PC_CROSS_MAX_SLOTS);
    PC_CHECK_ARG((uintptr_t)out % 4 == 0, "%s: out must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)ws % 8 == 0, "%s: ws must be 8-byte aligned", who);
    const size_t HW = (size_t)H * (size_t)W;
    const int cells = (P + 2) * (A + 2), bpf = cross_bpf((int64_t)HW);
    const int per = MAX_GRID / bpf;                                  // frames of one launch (a video is one launch; only a map of millions of frames is cut)
    for (int64_t c0 = 0; c0 < nf; c0 += per) {
        const int n = (int)(nf - c0 < per ? nf - c0 : per);
        const size_t fa = (size_t)f0 + (size_t)c0;
        CrossK k;
        k.pred = pred + fa * HW; k.truth = truth + fa * HW;
        k.ws = (int32_t*)ws + (size_t)c0 * (size_t)bpf * (size_t)cells;
        k.H = H; k.W = W; k.P = P; k.A = A; k.bpf = bpf;
        hipLaunchKernelGGL(crosstab_kernel, dim3((unsigned)(n * bpf)), dim3(BT), 0, (hipStream_t)s, k);
        PC_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(crosstab_fold_kernel, dim3((unsigned)n), dim3(BT), 0, (hipStream_t)s, (const int32_t*)k.ws, out + fa * (size_t)cells, cells, bpf,
                           (uint32_t)HW);
        PC_CHECK_LAUNCH(who);
    }
    return PC_OK;
}
