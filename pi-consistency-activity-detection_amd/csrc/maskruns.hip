// Masks and maps of ranks as row runs (detect.DetectEngine.mask_runs): the pixels of a pass leave the device as the maximal horizontal
// segments of equal non-zero byte value, a few hundred runs of 8 bytes for a frame of blobs instead of its H * W bytes.
//   pc_mask_run_index   the runs of every row of the frames f0 .. f0 + nf - 1 counted, then an exclusive prefix sum over the rows in raster
//                       order: run_count_kernel (grid over bands of BAND rows: the counts into `index`, the band's sum into `ws`),
//                       band_scan_kernel (ONE block scans the band sums in place and writes the total), band_add_kernel (a scan inside each
//                       band plus the band's offset, in place).
//   pc_mask_runs        run_write_kernel on the grid of the count: run index[r] + j is the j-th run of row r.
// The row walk is instances.hip's scan_rows with byte VALUES in place of foreground bits: a wave holds the loads of ROWS rows in flight, a
// 256-pixel segment that is all zero costs one ballot, and the neighbour across a lane or a segment boundary is a byte.  A lane's four pixels
// hold up to four starts and four ends (1, 2, 3, 4 are four runs), so the ranks inside the wave take four ballots each.
// No atomics, no floating point, nothing waits on another block (the three steps of the prefix sum are three launches), every loop's trip
// count is fixed before it starts, and every output word is a function of the input alone.
#include "common.h"
#include "rowbytes.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
constexpr int ROWS = 8;                      // rows a wave has in flight
constexpr int BAND = NW * ROWS;              // rows of one block of the count and of the write: the unit of the prefix sum across blocks
constexpr int MAX_ROWS = 1 << 24;            // the row field of a run
static_assert(BAND == 32 && 64 % BAND == 0, "band_add_kernel scans two bands per wave");
static_assert(PC_RUN_WORDS == 2, "a run is (row | value << 24, x0 | x1 << 16)");

struct RunK {
    const uint8_t* rows;                     // row 0 of the range: frame f0 of the map; the rows of consecutive frames follow each other
    int32_t* index; int32_t* ws; uint32_t* runs;
    long long cap;
    int R, W;                                // R = nf * H rows
};

// Wave `wv` of block b takes the rows b * BAND + wv * ROWS + j.  !WRITE: index[r] = the runs of row r, and the band's sum into ws[b].
// WRITE: run index[r] + k gets word 0 and x0 from its start, x1 from its end -- two 16-bit stores into word 1 -- if it lies below cap.
template <bool WRITE>
__global__ __launch_bounds__(256) void run_rows_kernel(const RunK p) {
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int R = p.R, W = p.W;
    const int r0 = (int)blockIdx.x * BAND + wv * ROWS;
    const int nseg = (W + 255) >> 8;
    int sb[ROWS], eb[ROWS], base[ROWS];
    uint32_t carry[ROWS];                                            // the last byte of the segment before: left neighbour of this one's first
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        sb[j] = eb[j] = 0;
        carry[j] = 0u;
        base[j] = (WRITE && r0 + j < R) ? p.index[r0 + j] : 0;
    }
    for (int g = 0; g < nseg; ++g) {
        const int x = (g << 8) + (lane << 2);
        uint32_t v[ROWS], after[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {                             // no branch here: addresses outside the row are moved to its first byte
            const int r = r0 + j;
            const bool in = r < R && x < W;
            const uint8_t* rp = p.rows + (size_t)(r < R ? r : 0) * (size_t)W;
            v[j] = map_bytes(rp + (in ? x : 0), in ? min(4, W - x) : 0);
            const bool last = in && lane == 63 && x + 4 < W;         // the right neighbour of the segment's last pixel
            const uint32_t a = rp[last ? x + 4 : 0];
            after[j] = last ? a : 0u;
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int r = r0 + j;
            if (r >= R) continue;                                    // the same in every lane of the wave
            if (__ballot(v[j] != 0u) == 0ull) { carry[j] = 0u; continue; }      // an all-zero segment (the same in every lane)
            const uint32_t w = v[j];
            // the neighbours across the lanes: the last byte of the lane before, the first of the lane after
            const uint32_t up = (uint32_t)__shfl_up((int)(w >> 24), 1, 64), dn = (uint32_t)__shfl_down((int)(w & 0xffu), 1, 64);
            const uint32_t prev = lane > 0 ? up : carry[j];
            const uint32_t next = lane < 63 ? dn : after[j];
            carry[j] = (uint32_t)__shfl((int)(w >> 24), 63, 64);
            const uint32_t left = (w << 8) | prev, right = (w >> 8) | (next << 24);      // byte e: the pixel left / right of pixel e
            uint32_t st = 0u, en = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t b = (w >> (8 * e)) & 0xffu;
                st |= (uint32_t)(b != 0u && ((left >> (8 * e)) & 0xffu) != b) << e;
                en |= (uint32_t)(b != 0u && ((right >> (8 * e)) & 0xffu) != b) << e;
            }
            const int ns = __popc(st), ne = __popc(en);
            int ts = 0, te = 0, sbelow = 0, ebelow = 0;
#pragma unroll
            for (int k = 1; k <= 4; ++k) {
                const unsigned long long ms = __ballot(ns >= k);
                ts += __popcll(ms);
                if (WRITE) {
                    const unsigned long long me = __ballot(ne >= k);
                    te += __popcll(me);
                    sbelow += lanes_below(ms);
                    ebelow += lanes_below(me);
                }
            }
            if (WRITE) {
                long long si = (long long)base[j] + sb[j] + sbelow, ei = (long long)base[j] + eb[j] + ebelow;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((st >> e) & 1u) {
                        if (si < p.cap) {
                            p.runs[(size_t)si * PC_RUN_WORDS] = (uint32_t)r | (((w >> (8 * e)) & 0xffu) << 24);
                            ((uint16_t*)(p.runs + (size_t)si * PC_RUN_WORDS + 1))[0] = (uint16_t)(x + e);
                        }
                        ++si;
                    }
                    if ((en >> e) & 1u) {
                        if (ei < p.cap) ((uint16_t*)(p.runs + (size_t)ei * PC_RUN_WORDS + 1))[1] = (uint16_t)(x + e + 1);
                        ++ei;
                    }
                }
            }
            sb[j] += ts; eb[j] += te;
        }
    }
    if (!WRITE) {
        int s = 0;
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            if (lane == 0 && r0 + j < R) p.index[r0 + j] = sb[j];
            s += sb[j];                                              // 0 for a row past the range
        }
        if (lane == 0) wsum[wv] = s;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += wsum[w];
            p.ws[blockIdx.x] = t;
        }
    }
}

// One block: ws[b] (the runs of band b) -> the runs of the bands before b, BT bands per trip with the carry of the trips before;
// index[R] = the total.
__global__ __launch_bounds__(256) void band_scan_kernel(int32_t* ws, int nb, int32_t* total_out) {
    __shared__ int wsum[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int trips = (nb + BT - 1) / BT;
    int carry = 0;
    for (int t = 0; t < trips; ++t) {
        const int i = t * BT + tid;
        const int v = i < nb ? ws[i] : 0;
        const int inc = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        int off = carry + inc - v, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (w < wv) off += wsum[w];
            tot += wsum[w];
        }
        if (i < nb) ws[i] = off;
        carry += tot;
        __syncthreads();                                             // wsum is written again in the next trip
    }
    if (tid == 0) *total_out = carry;
}

// One thread per row: index[r] (the runs of row r) -> the runs of the rows before it.  A wave holds two bands; the scan inside a band is the
// wave's scan minus what the wave's first band holds, the band's own offset comes from ws.  Every thread reads and writes its own row only.
__global__ __launch_bounds__(256) void band_add_kernel(int32_t* index, const int32_t* ws, int R) {
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * BT + (int)threadIdx.x;
    const int v = r < R ? index[r] : 0;
    const int inc = wave_incl_scan(v, lane);
    const int first = __shfl(inc, BAND - 1, 64);
    int ex = inc - v;
    if (lane >= BAND) ex -= first;
    if (r < R) index[r] = ex + ws[r / BAND];
}

int check_range(const char* who, const uint8_t* map, int F, int H, int W, int f0, int nf) {
    PC_CHECK_ARG(map, "%s: map is null", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of H = %d x W = %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG(W <= 65535, "%s: W = %d columns, more than the 65535 that x1 holds in 16 bits", who, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG((int64_t)nf * H <= MAX_ROWS, "%s: nf * H = %lld rows, more than the 2^24 the row field of a run holds", who, (long long)nf * H);
    PC_CHECK_ARG((int64_t)nf * H * W < (1ll << 31), "%s: nf * H * W = %lld pixels, a run count must stay below 2^31 (export a longer video in ranges)",
                 who, (long long)nf * H * W);
    return PC_OK;
}

}  // namespace

extern "C" int64_t pc_mask_run_ws_bytes(int nf, int H) {
    if (nf < 1 || H < 1 || (int64_t)nf * H > MAX_ROWS) return -1;
    return (int64_t)cdiv((int64_t)nf * H, BAND) * 4;
}

extern "C" int pc_mask_run_index(const uint8_t* map, int F, int H, int W, int f0, int nf, int32_t* index, void* ws, pc_stream s) {
    const char* who = "pc_mask_run_index";
    if (int rc = check_range(who, map, F, H, W, f0, nf)) return rc;
    PC_CHECK_ARG(index, "%s: index is null", who);
    PC_CHECK_ARG(ws, "%s: ws is null", who);
    PC_CHECK_ARG((uintptr_t)index % 4 == 0, "%s: index must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)ws % 4 == 0, "%s: ws must be 4-byte aligned", who);
    RunK k;
    k.rows = map + (size_t)f0 * (size_t)H * (size_t)W;
    k.index = index; k.ws = (int32_t*)ws; k.runs = nullptr; k.cap = 0;
    k.R = nf * H; k.W = W;
    const int nb = cdiv(k.R, BAND);
    hipLaunchKernelGGL(run_rows_kernel<false>, dim3((unsigned)nb), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(band_scan_kernel, dim3(1), dim3(BT), 0, (hipStream_t)s, k.ws, nb, index + k.R);
    PC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(band_add_kernel, dim3((unsigned)cdiv(k.R, BT)), dim3(BT), 0, (hipStream_t)s, index, (const int32_t*)k.ws, k.R);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

extern "C" int pc_mask_runs(const uint8_t* map, int F, int H, int W, int f0, int nf, const int32_t* index, int64_t cap, uint32_t* runs,
                            pc_stream s) {
    const char* who = "pc_mask_runs";
    if (int rc = check_range(who, map, F, H, W, f0, nf)) return rc;
    PC_CHECK_ARG(index, "%s: index is null", who);
    PC_CHECK_ARG(cap >= 0, "%s: cap = %lld below 0", who, (long long)cap);
    PC_CHECK_ARG(runs || cap == 0, "%s: runs is null with cap = %lld", who, (long long)cap);
    PC_CHECK_ARG((uintptr_t)index % 4 == 0, "%s: index must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)runs % 4 == 0, "%s: runs must be 4-byte aligned", who);
    RunK k;
    k.rows = map + (size_t)f0 * (size_t)H * (size_t)W;
    k.index = const_cast<int32_t*>(index); k.ws = nullptr; k.runs = runs; k.cap = cap;
    k.R = nf * H; k.W = W;
    hipLaunchKernelGGL(run_rows_kernel<true>, dim3((unsigned)cdiv(k.R, BAND)), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
