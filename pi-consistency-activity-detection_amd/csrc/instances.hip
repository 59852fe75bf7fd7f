// Per-frame instances on the device: the masks pc_detect_frames* leave (uint8 [F][H][W], video order, full-frame coordinates) split into
// connected components, ranked by area, specks dropped -- what a caller had to copy every mask to the host and label there for.
//   pc_frame_instances   one 256-thread block per frame, run-based labelling in LDS: the row runs (maximal horizontal foreground segments)
//                        in raster order, labels as minima over adjacent runs with pointer jumping, area and box per root, K rounds of block
//                        arg-max; optionally the map of ranks.  Latency-bound (F blocks on 256 CUs, a 240 x 320 frame is 77 KB and stays in
//                        L2): nothing here is tuned for bandwidth.
// Integer LDS atomics only; no global atomics, no floating point, nothing between blocks, no spin-waits.  The fixed point of the labelling
// (every run holds the smallest run index of its component) is unique, so a record does not depend on scheduling although reads inside an
// iteration race with writes: a label only decreases and never leaves its component.  Every loop's trip count is fixed before it starts; the
// labelling loop has the explicit bound n_runs + 1 (synchronous propagation reaches distance k after k iterations and a component's diameter
// is below n_runs) and a frame that hits it is reported as overflow, not looped on.
#include "common.h"
#include "rowbytes.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
constexpr int MAXR = PC_INST_MAX_RUNS, MAXROWS = PC_INST_MAX_ROWS;
constexpr int HDR = PC_INST_HDR, SLOT = PC_INST_WORDS;
static_assert(MAXROWS == BT * 8, "the row prefix sum gives every thread eight rows");
static_assert(MAXR <= 65536 && MAXROWS <= 65536, "run rows and columns are held as uint16");
// static LDS: 3 uint16 + 5 int32 per run, the row table, the reduction scratch
static_assert(MAXR * (3 * 2 + 5 * 4) + (MAXROWS + 1) * 4 + 256 <= 64 * 1024, "static LDS of frame_instances_kernel above 64 KiB");

struct InstK {
    const uint8_t* mask; int32_t* inst; uint8_t* imap;
    int H, W, f0, conn, min_area, K;
};

// One wave walks ROWS rows at a time (rows y0, y0 + NW, ...: the wave's next ones) in segments of 256 pixels, four per lane; the loads of all
// ROWS rows are issued before the first is looked at (a wave that waits for each row's bytes before asking for the next spends its time
// waiting), and a segment without foreground costs one ballot.  A pixel
// starts a run iff it is foreground and its left neighbour is not, and ends one iff its right neighbour is not: both are decided per pixel
// from the row itself, so a run that crosses a lane's or a segment's boundary is one run, and the j-th start and the j-th end of a row belong
// to the same run.  WRITE: run `rowstart[y] + j` gets x0 / row from its start and x1 from its end; otherwise rowstart[y] = the runs of row y.
constexpr int ROWS = 8;

template <bool WRITE>
__device__ __forceinline__ void scan_rows(const uint8_t* __restrict__ mf, int H, int W, int y0, int lane, int* rowstart, uint16_t* rx0,
                                          uint16_t* rx1, uint16_t* rrow) {
    const int nseg = (W + 255) >> 8;
    int sb[ROWS], eb[ROWS], base[ROWS];
    uint32_t carry[ROWS];                                            // the last pixel of the segment before: left neighbour of this one's first
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int y = y0 + j * NW;
        sb[j] = eb[j] = 0;
        carry[j] = 0;
        base[j] = (WRITE && y < H) ? rowstart[y] : 0;
    }
    for (int g = 0; g < nseg; ++g) {
        const int x = (g << 8) + (lane << 2);
        uint32_t b[ROWS], after[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {                             // no branch here: addresses outside the row are moved to its first byte
            const int y = y0 + j * NW;
            const bool in = y < H && x < W;
            const uint8_t* rp = mf + (size_t)(y < H ? y : 0) * W;
            b[j] = fg_bits(rp + (in ? x : 0), in ? min(4, W - x) : 0);
            const bool last = in && lane == 63 && x + 4 < W;         // the right neighbour of the segment's last pixel
            after[j] = last & (rp[last ? x + 4 : 0] != 0);
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int y = y0 + j * NW;
            if (y >= H) continue;                                    // the same in every lane of the wave
            if (__ballot(b[j] != 0u) == 0ull) { carry[j] = 0; continue; }     // no foreground in the segment (the same in every lane)
            // the neighbours across the lanes: the last pixel of the lane before, the first of the lane after
            const unsigned long long m0 = __ballot(b[j] & 1u), m3 = __ballot((b[j] >> 3) & 1u);
            const uint32_t prev = lane > 0 ? (uint32_t)(m3 >> (lane - 1)) & 1u : carry[j];
            const uint32_t next = lane < 63 ? (uint32_t)(m0 >> (lane + 1)) & 1u : after[j];
            carry[j] = (uint32_t)(m3 >> 63);
            const uint32_t ext = prev | (b[j] << 1) | (next << 5);   // bit e: the pixel left of pixel e; bit e + 2: the one right of it
            const uint32_t st = b[j] & ~ext & 0xfu, en = b[j] & ~(ext >> 2) & 0xfu;
            // starts and ends in the lanes below, and in the wave: ballots and bit counts, no trip through LDS.  Four pixels hold at most two
            // starts and two ends.
            const int ns = __popc(st), ne = __popc(en);
            const unsigned long long s1 = __ballot(ns >= 1), s2 = __ballot(ns >= 2), e1 = __ballot(ne >= 1), e2 = __ballot(ne >= 2);
            const int ts = __popcll(s1) + __popcll(s2), te = __popcll(e1) + __popcll(e2);
            if (WRITE) {
                int si = base[j] + sb[j] + lanes_below(s1) + lanes_below(s2), ei = base[j] + eb[j] + lanes_below(e1) + lanes_below(e2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((st >> e) & 1u) { if (si < MAXR) { rx0[si] = (uint16_t)(x + e); rrow[si] = (uint16_t)y; } ++si; }
                    if ((en >> e) & 1u) { if (ei < MAXR) rx1[ei] = (uint16_t)(x + e + 1); ++ei; }
                }
            }
            sb[j] += ts; eb[j] += te;
        }
    }
    if (!WRITE && lane == 0) {
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (y0 + j * NW < H) rowstart[y0 + j * NW] = sb[j];
    }
}

// grid (nf): block b is frame f0 + b.
__global__ __launch_bounds__(256) void frame_instances_kernel(const InstK p) {
    __shared__ uint16_t rx0[MAXR], rx1[MAXR], rrow[MAXR];            // run i: row rrow[i], columns [rx0[i], rx1[i]); raster order
    __shared__ int label[MAXR];
    __shared__ int area[MAXR], xmin[MAXR], xmax[MAXR], ymax[MAXR];   // per root; area < 0: the root has rank -area - 1
    __shared__ int rowstart[MAXROWS + 1];                            // the runs of row y are rowstart[y] .. rowstart[y + 1] - 1
    __shared__ int wsum[NW];
    __shared__ unsigned long long red[2][NW];
    __shared__ int ncomp_sh;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int H = p.H, W = p.W, K = p.K;
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    const size_t f = (size_t)p.f0 + blockIdx.x;
    const uint8_t* __restrict__ mf = p.mask + f * HW;
    int32_t* rec = p.inst + f * (size_t)(HDR + K * SLOT);
    uint8_t* __restrict__ im = p.imap ? p.imap + f * HW : nullptr;

    // ---- runs: count per row, prefix sum over the rows, write
    for (int y = wv; y < H; y += NW * ROWS) scan_rows<false>(mf, H, W, y, lane, rowstart, rx0, rx1, rrow);
    __syncthreads();
    int v[8], s = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int y = tid * 8 + j;
        v[j] = y < H ? rowstart[y] : 0;
        s += v[j];
    }
    const int inc = wave_incl_scan(s, lane);
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int off = inc - s, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wv) off += wsum[w];
        total += wsum[w];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int y = tid * 8 + j;
        if (y < H) rowstart[y] = off;
        off += v[j];
    }
    if (tid == 0) rowstart[H] = total;
    __syncthreads();

    bool over = total > MAXR;                                        // the same in every thread, here and below
    const int n = over ? 0 : total;
    if (!over) {
        for (int y = wv; y < H; y += NW * ROWS) scan_rows<true>(mf, H, W, y, lane, rowstart, rx0, rx1, rrow);
        for (int i = tid; i < n; i += BT) label[i] = i;
        __syncthreads();
        // ---- labels: minima over the adjacent runs of the rows above and below, one pointer jump, until nothing changes
        const int slack = p.conn == 8 ? 1 : 0;                       // 4: a0 < b1 && b0 < a1; 8: a0 <= b1 && b0 <= a1
        bool settled = false;
        for (int it = 0; it <= n; ++it) {
            int ch = 0;
            for (int i = tid; i < n; i += BT) {
                const int a0 = rx0[i], a1 = rx1[i] + slack, y = rrow[i], l = label[i];
                int m = l;
                if (y > 0) {
                    const int j1 = rowstart[y];
                    for (int j = rowstart[y - 1]; j < j1; ++j)
                        if (a0 < (int)rx1[j] + slack && (int)rx0[j] < a1) m = min(m, label[j]);
                }
                if (y + 1 < H) {
                    const int j1 = rowstart[y + 2];
                    for (int j = rowstart[y + 1]; j < j1; ++j)
                        if (a0 < (int)rx1[j] + slack && (int)rx0[j] < a1) m = min(m, label[j]);
                }
                m = min(m, label[m]);
                if (m < l) { label[i] = m; ch = 1; }
            }
            if (!__syncthreads_or(ch)) { settled = true; break; }
        }
        over = !settled;
    }

    if (over) {
        if (tid == 0) { rec[0] = 0; rec[1] = 0; rec[2] = total; rec[3] = 1; }
        for (int t = tid; t < K * SLOT; t += BT) rec[HDR + t] = 0;
    } else {
        // ---- area and box per root
        for (int i = tid; i < n; i += BT) { area[i] = 0; xmin[i] = 0x7fffffff; xmax[i] = 0; ymax[i] = 0; }
        if (tid == 0) ncomp_sh = 0;
        __syncthreads();
        for (int i = tid; i < n; i += BT) {
            const int r = label[i], a0 = rx0[i], a1 = rx1[i];
            atomicAdd(&area[r], a1 - a0);
            atomicMin(&xmin[r], a0);
            atomicMax(&xmax[r], a1);
            atomicMax(&ymax[r], (int)rrow[i] + 1);
        }
        __syncthreads();
        int cnt = 0;
        for (int i = tid; i < n; i += BT) cnt += area[i] >= p.min_area;      // a run that is no root keeps area 0 < min_area
        if (cnt) atomicAdd(&ncomp_sh, cnt);
        __syncthreads();
        const int ncomp = ncomp_sh, kept = min(ncomp, K);
        if (tid == 0) { rec[0] = ncomp; rec[1] = kept; rec[2] = total; rec[3] = 0; }
        for (int t = tid; t < K * SLOT; t += BT)
            if (t / SLOT >= kept) rec[HDR + t] = 0;
        // ---- kept rounds of arg-max by (area descending, first pixel ascending): a root is the first run of its component in raster order, so
        // the smaller root index is the smaller first pixel
        for (int r = 0; r < kept; ++r) {
            unsigned long long best = 0;
            for (int i = tid; i < n; i += BT) {
                const int a = area[i];
                if (a >= p.min_area) {
                    const unsigned long long key = ((unsigned long long)(uint32_t)a << 32) | (0xffffffffu - (uint32_t)i);
                    best = key > best ? key : best;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), o, 64), lo = __shfl_xor((uint32_t)best, o, 64);
                const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                best = other > best ? other : best;
            }
            if (lane == 0) red[r & 1][wv] = best;
            __syncthreads();                                         // red[r & 1] is written again two rounds on, behind the next round's barrier
            best = red[r & 1][0];
#pragma unroll
            for (int w = 1; w < NW; ++w) best = red[r & 1][w] > best ? red[r & 1][w] : best;
            const int w = (int)(0xffffffffu - (uint32_t)best);
            if (w >= 0 && w < n && (w & (BT - 1)) == tid) {          // the thread that scans root w: its own next scan sees the mark
                int32_t* q = rec + HDR + r * SLOT;
                q[0] = area[w]; q[1] = xmin[w]; q[2] = rrow[w]; q[3] = xmax[w]; q[4] = ymax[w]; q[5] = (int)rrow[w] * W + (int)rx0[w];
                area[w] = -(r + 1);
            }
        }
        __syncthreads();
    }

    // ---- the map of ranks: the frame in groups of four consecutive pixels, the run of a foreground pixel by bisection in its row; a thread
    // has the loads of four groups in flight
    if (im) {
        const uint32_t total4 = (HW + 3u) >> 2;
        for (uint32_t g0 = tid; g0 < total4; g0 += BT * 4) {
            uint32_t bits[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = g0 + u * BT, px = g << 2;
                const bool in = g < total4;
                bits[u] = fg_bits(mf + (in ? px : 0u), in ? (int)(HW - px < 4u ? HW - px : 4u) : 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = g0 + u * BT, px = g << 2;
                if (g >= total4) continue;
                const int ny = (int)(HW - px < 4u ? HW - px : 4u);
                const uint32_t b = bits[u];
                int y = (int)(px / (uint32_t)W), x = (int)(px - (uint32_t)y * (uint32_t)W);
                uint32_t out = 0, cval = 255u;
                int cy = -1, cx1 = 0;                                    // the run found last: row, end, value
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((b >> e) & 1u) {
                        uint32_t val = 255u;
                        if (!over) {
                            if (!(y == cy && x < cx1)) {                 // not the run the pixel before it lay in
                                int lo = rowstart[y], hi = rowstart[y + 1];
                                for (int step = hi - lo > 1 ? 32 - __clz(hi - lo - 1) : 0; step > 0; --step) {    // at most 11: 2^11 = PC_INST_MAX_RUNS
                                    const int mid = (lo + hi) >> 1;
                                    if (hi - lo > 1) { if ((int)rx0[mid] <= x) lo = mid; else hi = mid; }
                                }
                                lo = min(lo, MAXR - 1);
                                const int a = area[label[lo]];
                                cy = y; cx1 = rx1[lo]; cval = a < 0 ? (uint32_t)(-a) : 255u;
                            }
                            val = cval;
                        }
                        out |= val << (8 * e);
                    }
                    if (++x == W) { x = 0; ++y; }
                }
                uint8_t* q = im + px;
                if (ny == 4 && ((uintptr_t)q & 3) == 0) {
                    *(uint32_t*)q = out;
                } else {
                    for (int e = 0; e < ny; ++e) q[e] = (uint8_t)(out >> (8 * e));
                }
            }
        }
    }
}

}  // namespace

extern "C" int pc_frame_instances(const uint8_t* mask, int F, int H, int W, int f0, int nf, int conn, int min_area, int K, int32_t* inst,
                                  uint8_t* imap, pc_stream s) {
    const char* who = "pc_frame_instances";
    PC_CHECK_ARG(mask && inst, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a mask holds", who, F, H, W);
    PC_CHECK_ARG(H <= PC_INST_MAX_ROWS, "%s: H = %d rows, more than the %d of the row table", who, H, PC_INST_MAX_ROWS);
    PC_CHECK_ARG(W <= 65535, "%s: W = %d columns, more than 65535", who, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are outside the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the mask", who, f0, nf, F);
    PC_CHECK_ARG(conn == 4 || conn == 8, "%s: conn = %d, 4 or 8", who, conn);
    PC_CHECK_ARG(min_area >= 1, "%s: min_area = %d below 1", who, min_area);
    PC_CHECK_ARG(K >= 1 && K <= 32, "%s: K = %d outside 1..32", who, K);
    PC_CHECK_ARG((uintptr_t)inst % 4 == 0, "%s: inst must be 4-byte aligned", who);
    InstK k;
    k.mask = mask; k.inst = inst; k.imap = imap;
    k.H = H; k.W = W; k.f0 = f0; k.conn = conn; k.min_area = min_area; k.K = K;
    hipLaunchKernelGGL(frame_instances_kernel, dim3((unsigned)nf), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

// ---------------------------------------------------------------------- a confidence per instance (detect.DetectEngine, instance_scores)
//   pc_instance_scores   the map of ranks pc_frame_instances leaves and the uint16 probability map pc_frame_probs (detect.hip) leaves, reduced
//                        per instance: for every slot the 64-bit sum of its pixels' probabilities and their number.  One 256-thread block
//                        per frame, latency-bound as the labelling is.  Integer addition only -- per-wave LDS bins, then folded -- so the
//                        record is the same bits in whatever order the adds land; no global atomics, nothing to zero.
namespace {

constexpr int SWORDS = PC_SCORE_WORDS, MAXSLOTS = 32 + 1;            // K <= 32 ranks and the slot of all other foreground

struct ScoreK {
    const uint8_t* imap; const uint16_t* prob; int32_t* out;
    int H, W, f0, K;
};

// grid (nf): block b is frame f0 + b.  A thread walks the frame's groups of four consecutive pixels (the loads of four groups in flight, as the
// map's writer has them), keeps the sum and count of the slot it is in and flushes them into its wave's bins when the slot changes.  The
// probability of a background pixel is never read: a group of four foreground pixels at an 8-byte address comes as one load, anything else
// pixel by pixel.
__global__ __launch_bounds__(256) void instance_scores_kernel(const ScoreK p) {
    __shared__ unsigned long long bsum[NW][MAXSLOTS];
    __shared__ int bcnt[NW][MAXSLOTS];
    const int tid = threadIdx.x, wv = tid >> 6, K = p.K;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W, total4 = (HW + 3u) >> 2;
    const size_t f = (size_t)p.f0 + blockIdx.x;
    const uint8_t* __restrict__ im = p.imap + f * HW;
    const uint16_t* __restrict__ pf = p.prob + f * HW;
    for (int t = tid; t < NW * MAXSLOTS; t += BT) { (&bsum[0][0])[t] = 0ull; (&bcnt[0][0])[t] = 0; }
    __syncthreads();

    int cur = -1, cnt = 0;                                           // the slot the thread is in; nothing to flush while cnt == 0
    unsigned long long sum = 0ull;
    for (uint32_t g0 = tid; g0 < total4; g0 += BT * 4) {
        uint32_t vals[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t g = g0 + u * BT, px = g << 2;
            const bool in = g < total4;
            vals[u] = map_bytes(im + (in ? px : 0u), in ? (int)(HW - px < 4u ? HW - px : 4u) : 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t v4 = vals[u];
            if (v4 == 0u) continue;                                  // background (or a group past the frame's end): nothing read
            const uint32_t px = (g0 + u * BT) << 2;
            const uint16_t* q = pf + px;
            uint32_t qv[4] = {0u, 0u, 0u, 0u};
            const bool all = (v4 & 0xffu) && (v4 & 0xff00u) && (v4 & 0xff0000u) && (v4 & 0xff000000u);      // then the group has four pixels
            if (all && ((uintptr_t)q & 7) == 0) {
                const uint2 w = *(const uint2*)q;
                qv[0] = w.x & 0xffffu; qv[1] = w.x >> 16; qv[2] = w.y & 0xffffu; qv[3] = w.y >> 16;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((v4 >> (8 * e)) & 0xffu) qv[e] = q[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = (int)((v4 >> (8 * e)) & 0xffu);
                if (v == 0) continue;
                const int slot = v <= K ? v - 1 : K;
                if (slot != cur) {
                    if (cnt) { atomicAdd(&bsum[wv][cur], sum); atomicAdd(&bcnt[wv][cur], cnt); }
                    cur = slot; sum = 0ull; cnt = 0;
                }
                sum += qv[e]; ++cnt;
            }
        }
    }
    if (cnt) { atomicAdd(&bsum[wv][cur], sum); atomicAdd(&bcnt[wv][cur], cnt); }
    __syncthreads();
    if (tid <= K) {
        unsigned long long s = bsum[0][tid];
        int n = bcnt[0][tid];
#pragma unroll
        for (int w = 1; w < NW; ++w) { s += bsum[w][tid]; n += bcnt[w][tid]; }
        int32_t* o = p.out + (f * (size_t)(K + 1) + (size_t)tid) * SWORDS;
        o[0] = (int32_t)(uint32_t)s; o[1] = (int32_t)(uint32_t)(s >> 32); o[2] = n;
    }
}

}  // namespace

extern "C" int pc_instance_scores(const uint8_t* imap, const uint16_t* prob, int F, int H, int W, int f0, int nf, int K, int32_t* out, pc_stream s) {
    const char* who = "pc_instance_scores";
    PC_CHECK_ARG(imap && prob && out, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG(K >= 1 && K <= 32, "%s: K = %d outside 1..32", who, K);
    PC_CHECK_ARG((uintptr_t)prob % 2 == 0 && (uintptr_t)out % 4 == 0, "%s: prob must be 2-byte and out 4-byte aligned", who);
    ScoreK k;
    k.imap = imap; k.prob = prob; k.out = out;
    k.H = H; k.W = W; k.f0 = f0; k.K = K;
    hipLaunchKernelGGL(instance_scores_kernel, dim3((unsigned)nf), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

// ---------------------------------------------------------------------- mask overlaps between frames (detect.DetectEngine, instance_links)
//   pc_instance_overlaps  the map of ranks pc_frame_instances leaves, histogrammed per pair of frames: for frame f and each lag l the number
//                         of pixels that slot a of frame f shares with slot b of frame f + l + 1 -- what linking per-actor tubes by mask
//                         overlap needs, and what a caller had to copy every map to the host for.  One 256-thread block per (frame, lag),
//                         latency-bound as its siblings are.  Integer addition only -- per-wave LDS bins, then folded -- so the record is the
//                         same bits in whatever order the adds land; no global atomics, nothing to zero.
namespace {

constexpr int MAXPAIRS = MAXSLOTS * MAXSLOTS;
static_assert(NW * MAXPAIRS * 4 == 17424, "static LDS of instance_overlaps_kernel");

struct OverlapK {
    const uint8_t* imap; int32_t* out;
    int F, H, W, f0, K, L;
};

// grid (nf, L): block (b, l) is frame f0 + b against frame f0 + b + l + 1.  A thread walks the groups of four consecutive pixels of the first
// frame (the loads of four groups in flight); the partner's bytes of a group are read only where the first frame holds foreground.  The two
// frames lie H * W bytes apart, so for odd H * W their groups sit differently in their dwords: each side goes through map_bytes on its own.
// The thread keeps a count for the (a, b) pair it is in and flushes it into its wave's bins when the pair changes.
__global__ __launch_bounds__(256) void instance_overlaps_kernel(const OverlapK p) {
    __shared__ int bins[NW][MAXPAIRS];
    const int tid = threadIdx.x, wv = tid >> 6, K = p.K, S = K + 1, cells = S * S;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)p.W, total4 = (HW + 3u) >> 2;
    const size_t f = (size_t)p.f0 + blockIdx.x, g = f + blockIdx.y + 1;
    int32_t* o = p.out + (f * (size_t)p.L + blockIdx.y) * (size_t)cells;
    if (g >= (size_t)p.F) {                                          // no partner frame (the same in every thread): the lag's cells are zeros
        for (int t = tid; t < cells; t += BT) o[t] = 0;
        return;
    }
    const uint8_t* __restrict__ ia = p.imap + f * HW;
    const uint8_t* __restrict__ ib = p.imap + g * HW;
    for (int w = 0; w < NW; ++w)
        for (int t = tid; t < cells; t += BT) bins[w][t] = 0;
    __syncthreads();

    int cur = -1, cnt = 0;                                           // the pair the thread is in; nothing to flush while cnt == 0
    for (uint32_t g0 = tid; g0 < total4; g0 += BT * 4) {
        uint32_t va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t gr = g0 + u * BT, px = gr << 2;
            const bool in = gr < total4;
            va[u] = map_bytes(ia + (in ? px : 0u), in ? (int)(HW - px < 4u ? HW - px : 4u) : 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            vb[u] = 0u;
            if (va[u] == 0u) continue;                               // background (or a group past the frame's end): the partner is not read
            const uint32_t px = (g0 + u * BT) << 2;
            vb[u] = map_bytes(ib + px, (int)(HW - px < 4u ? HW - px : 4u));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (va[u] == 0u || vb[u] == 0u) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int a = (int)((va[u] >> (8 * e)) & 0xffu), b = (int)((vb[u] >> (8 * e)) & 0xffu);
                if (a == 0 || b == 0) continue;
                const int pair = (a <= K ? a - 1 : K) * S + (b <= K ? b - 1 : K);
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
    for (int t = tid; t < cells; t += BT) {
        int n = bins[0][t];
#pragma unroll
        for (int w = 1; w < NW; ++w) n += bins[w][t];
        o[t] = n;
    }
}

}  // namespace

extern "C" int pc_instance_overlaps(const uint8_t* imap, int F, int H, int W, int f0, int nf, int K, int L, int32_t* out, pc_stream s) {
    const char* who = "pc_instance_overlaps";
    PC_CHECK_ARG(imap && out, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG(K >= 1 && K <= 32, "%s: K = %d outside 1..32", who, K);
    PC_CHECK_ARG(L >= 1 && L <= PC_LINK_MAX_LAGS, "%s: L = %d outside 1..%d", who, L, PC_LINK_MAX_LAGS);
    PC_CHECK_ARG((uintptr_t)out % 4 == 0, "%s: out must be 4-byte aligned", who);
    OverlapK k;
    k.imap = imap; k.out = out;
    k.F = F; k.H = H; k.W = W; k.f0 = f0; k.K = K; k.L = L;
    hipLaunchKernelGGL(instance_overlaps_kernel, dim3((unsigned)nf, (unsigned)L), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
