// The kept probability map of a pass cut at a threshold word (detect.DetectEngine.set_mask_threshold / recut): per frame the mask q >= word
// and words 0..5 of the record -- count, half-open box, score -- so that everything behind a mask runs on a cut at any threshold unchanged.
//   pc_prob_cut   prob_cut_kernel on a grid of bpf blocks per frame (det_views_bpf: a function of H * W alone, at most 64): each block strides
//                 over its share of the frame's four-pixel groups, writes their mask bytes (store_mask4) and leaves one Partial in `ws`
//                 (FrameAcc::block_partial); prob_cut_records_kernel, one thread per frame, adds the partials in block order
//                 (record_count_box) and divides once.  Words 6 and 7 of a record are the detect entries' and are not written.
// The walk is prob_hist_kernel's: the loads of four groups in flight, the four probabilities as one 8-byte load where the frame starts on an
// 8-byte address (prob_words), element by element otherwise and in a frame's tail group.
// "Positive at a word" is pc_prob_truth_hist's q >= word, so a sweep and a cut cannot disagree on a pixel.
// The score's numerator is the sum of the probability WORDS of the positive pixels.  It travels in FrameAcc's double: a word is an integer
// below 2^16 and a frame holds fewer than 2^31 pixels, so every partial sum, in any order, is an integer below 2^47 < 2^53 and every
// addition is exact -- the sum is the integer sum, the same bits whichever way the blocks and lanes are folded.  The one floating-point
// operation that rounds is the final division (float)(S / (65535.0 * c)), whose divisor is exact as well.
// No global atomics, nothing waits on another block (the records are a launch of their own), every loop's trip count is known before it
// starts, every output word is a function of the input alone.
#include "detectrec.h"
#include "probwords.h"

namespace {

constexpr int MAX_GRID = 1 << 23;                                    // blocks of one launch: 2^31 threads

struct CutK {
    const uint16_t* prob; uint8_t* mask;                             // frame 0 of the launch's frames; mask may be null
    Partial* part;                                                   // [frame][bpf] of the launch's frames
    int H, W, bpf;
    uint32_t word;
};

// grid (frames * bpf): block x is share x % bpf of frame x / bpf.  The bpf blocks of a frame stride over its groups of four consecutive
// pixels; a group past the frame's end is neither read nor written.
__global__ __launch_bounds__(256) void prob_cut_kernel(const CutK p) {
    const int tid = threadIdx.x, W = p.W;
    const uint32_t word = p.word;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)W, total4 = (HW + 3u) >> 2;
    const uint32_t fr = blockIdx.x / (uint32_t)p.bpf, part = blockIdx.x % (uint32_t)p.bpf, stride = (uint32_t)p.bpf * BT;
    const uint16_t* __restrict__ pp = p.prob + (size_t)fr * HW;
    uint8_t* mf = p.mask ? p.mask + (size_t)fr * HW : nullptr;
    const bool wide = ((uintptr_t)pp & 7) == 0;                      // a group starts 8 * gr bytes into its frame

    FrameAcc acc;
    for (uint32_t g0 = part * BT + tid; g0 < total4; g0 += stride * 4) {
        uint2 va[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t gr = g0 + u * stride, px = gr << 2;
            const bool in = gr < total4;
            const int n = in ? (int)(HW - px < 4u ? HW - px : 4u) : 0;
            va[u] = prob_words(pp + (in ? px : 0u), n, wide);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t gr = g0 + u * stride, px = gr << 2;
            if (gr >= total4) continue;
            const int n = (int)(HW - px < 4u ? HW - px : 4u);
            const uint32_t q[4] = {va[u].x & 0xffffu, va[u].x >> 16, va[u].y & 0xffffu, va[u].y >> 16};
            uint32_t bits = 0;                                           // a pixel past the frame's end came as 0 < word
#pragma unroll
            for (int e = 0; e < 4; ++e) bits |= q[e] >= word ? 1u << (8 * e) : 0u;
            if (mf) store_mask4(mf + px, bits, n);
            if (bits == 0u) continue;
            const int gy = (int)(px / (uint32_t)W), gx = (int)(px - (uint32_t)gy * (uint32_t)W);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!((bits >> (8 * e)) & 1u)) continue;
                int y, x;
                group_pixel(gy, gx, e, W, y, x);
                acc.add((float)q[e], y, x);                              // exact: q < 2^16
            }
        }
    }
    acc.block_partial(p.part + blockIdx.x);
}

// one thread per frame of the launch: its partials in block order -> words 0..5 of its record
__global__ __launch_bounds__(256) void prob_cut_records_kernel(const Partial* __restrict__ part, int32_t* rec, int nframes, int bpf) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= nframes) return;
    const Partial* q = part + (size_t)t * bpf;
    FrameAcc a;
    for (int b = 0; b < bpf; ++b) a.add(q[b]);
    int32_t* r = rec + (size_t)t * REC_WORDS;
    const bool any = record_count_box(a, 0, 0, r);
    r[5] = __float_as_int(any ? (float)(a.sum / ((double)PC_PROB_ONE * (double)a.cnt)) : 0.0f);
}

}  // namespace

extern "C" int64_t pc_prob_cut_ws_bytes(int nf, int H, int W) {
    if (nf < 1 || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return -1;
    return (int64_t)nf * det_views_bpf((int64_t)H * W) * (int64_t)sizeof(Partial);
}

extern "C" int pc_prob_cut(const uint16_t* prob, int F, int H, int W, int f0, int nf, int word, uint8_t* mask, int32_t* rec, void* ws, pc_stream s) {
    const char* who = "pc_prob_cut";
    PC_CHECK_ARG(prob && rec && ws, "%s: null pointer (prob, rec or ws)", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG(word >= 1 && word <= PC_PROB_ONE, "%s: word = %d outside 1..%d", who, word, PC_PROB_ONE);
    PC_CHECK_ARG((uintptr_t)prob % 2 == 0, "%s: prob must be 2-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)rec % 4 == 0, "%s: rec must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)ws % 8 == 0, "%s: ws must be 8-byte aligned", who);
    const size_t HW = (size_t)H * (size_t)W;
    const int bpf = det_views_bpf((int64_t)HW);
    const int per = MAX_GRID / bpf;                                  // frames of one launch (a video is one launch; only a map of millions of frames is cut)
    CutK k;
    k.H = H; k.W = W; k.bpf = bpf; k.word = (uint32_t)word;
    for (int64_t c0 = 0; c0 < nf; c0 += per) {
        const int n = (int)(nf - c0 < per ? nf - c0 : per);
        const size_t fa = (size_t)f0 + (size_t)c0;
        k.prob = prob + fa * HW;
        k.mask = mask ? mask + fa * HW : nullptr;
        k.part = (Partial*)ws + (size_t)c0 * (size_t)bpf;
        hipLaunchKernelGGL(prob_cut_kernel, dim3((unsigned)(n * bpf)), dim3(BT), 0, (hipStream_t)s, k);
        PC_CHECK_LAUNCH(who);
        hipLaunchKernelGGL(prob_cut_records_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, (hipStream_t)s, (const Partial*)k.part,
                           rec + fa * REC_WORDS, n, bpf);
        PC_CHECK_LAUNCH(who);
    }
    return PC_OK;
}
