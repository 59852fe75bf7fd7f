// What the detection entries of detect.hip (pc_detect_frames, pc_detect_frames_views, pc_frame_probs), detectscale.hip
// (pc_detect_frames_scaled) and cliphop.hip (pc_clip_planes, pc_detect_frames_planes) do to a pixel and to a frame, each rule once, so that
// a mask byte, a probability or a record cannot mean two things:
//   Partial / DetectK       one block's share of a frame and the kernel arguments of the traversals and the records kernel
//   FrameAcc                a thread's share of a frame (sum, count, box): add a positive pixel, add a block's Partial, and block_partial,
//                           the end of every traversal kernel (thread -> wave -> block, a fixed order)
//   sigmoid / prob_word     the probability of a logit, and its uint16 (0 for a NaN)
//   store_mask4 / store_prob4   a group's mask bytes and probabilities, as one store where the address allows
//   slot_frame              which video frame a (clip, frame of the clip) slot of a launch is
//   merge_to_plane          a frame's merged logits (viewmerge.h: merge_group4) and cover counts into a padded plane
//   tap_row / detect_native_frame   the traversal of a native frame whose logits are bilinear taps of a plane, over a tap reader
//   record_count_box        a frame's accumulated share -> words 0..4 of its record (probcut.hip ends in it too)
//   record_from_partials    a frame's partials in block order -> its 8-word record
//   detect_records_kernel   the second launch of the clip-table entries
//   det_views_bpf, plane_stride, detect_args   host arithmetic and the argument checks, in the order they refuse
// Everything here has internal linkage: each translation unit that includes it gets its own copy of the kernels.
#pragma once
#include "common.h"
#include "evalpred.h"
#include "clipgeom.h"
#include "viewmerge.h"

namespace {

constexpr int BT = 256, NW = BT / 64;
constexpr int REC_WORDS = 8;

struct Partial {                 // one block's share of a frame, crop coordinates; 32 bytes
    double sum;                  // sum of sigmoid(x) over its positive pixels, in the fixed order thread -> wave -> block
    int32_t count, x0, y0, x1, y1, pad;      // closed box; count == 0: the box is (INT_MAX, INT_MAX, -1, -1)
};

struct DetectK {                 // both traversals: the centre one takes its crop from view 0 of the geometry
    const float* logits; uint8_t* mask; int32_t* rec; Partial* part;
    int row0, bpf;
    ClipGeom g;
};

__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// sg = sigmoid(v) as the uint16 probability; a NaN is 0, written as such and not left to the conversion
__device__ __forceinline__ uint32_t prob_word(float v, float sg) { return v == v ? __float2uint_rn(sg * (float)PC_PROB_ONE) : 0u; }

// The first ny mask bytes of a group (bit 8 * e of bits: pixel e is positive): one dword where the address allows -- a mask row starts at
// any byte address when W is odd --, bytes otherwise.
__device__ __forceinline__ void store_mask4(uint8_t* m, uint32_t bits, int ny) {
    if (ny == 4 && ((uintptr_t)m & 3) == 0) {
        *(uint32_t*)m = bits;
    } else {
        for (int e = 0; e < ny; ++e) m[e] = (uint8_t)((bits >> (8 * e)) & 1);
    }
}

// The first ny probabilities of a group: one 8-byte store where the address allows -- a frame of odd H * W starts at an odd element --,
// 2-byte stores otherwise.
__device__ __forceinline__ void store_prob4(uint16_t* o, const uint32_t q[4], int ny) {
    if (ny == 4 && ((uintptr_t)o & 7) == 0) {
        *(uint2*)o = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
    } else {
        for (int e = 0; e < ny; ++e) o[e] = (uint16_t)q[e];
    }
}

struct FrameAcc {
    double sum = 0.0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;

    __device__ __forceinline__ void add(float sg, int y, int x) {    // a positive pixel of probability sg
        sum += (double)sg;
        ++cnt;
        x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
    }

    __device__ __forceinline__ void add(const Partial& q) {
        sum += q.sum; cnt += q.count;
        x0 = min(x0, q.x0); y0 = min(y0, q.y0); x1 = max(x1, q.x1); y1 = max(y1, q.y1);
    }

    // The end of the traversal kernels: a thread's share of a frame -> the block's Partial.  Count and box through the wave by shuffles, the
    // four waves through LDS, thread 0 folds them in wave order.  Holds a block barrier: every thread of the block calls it.
    __device__ __forceinline__ void block_partial(Partial* out) {
        __shared__ double shs[NW];
        __shared__ int shi[NW][5];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        sum = wave_sum_d(sum);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
            x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
        }
        if (lane == 0) { shs[wv] = sum; shi[wv][0] = cnt; shi[wv][1] = x0; shi[wv][2] = y0; shi[wv][3] = x1; shi[wv][4] = y1; }
        __syncthreads();
        if (threadIdx.x == 0) {
            Partial q;
            q.sum = ((shs[0] + shs[1]) + shs[2]) + shs[3];
            q.count = shi[0][0]; q.x0 = shi[0][1]; q.y0 = shi[0][2]; q.x1 = shi[0][3]; q.y1 = shi[0][4]; q.pad = 0;
            for (int w = 1; w < NW; ++w) {
                q.count += shi[w][0];
                q.x0 = min(q.x0, shi[w][1]); q.y0 = min(q.y0, shi[w][2]); q.x1 = max(q.x1, shi[w][3]); q.y1 = max(q.y1, shi[w][4]);
            }
            *out = q;
        }
    }
};

// slot = clip * 8 + frame of the clip (blockIdx.y of the traversals) -> the video frame, or -1 for a frame past the end, of which nothing
// is read and nothing written
__device__ __forceinline__ int64_t slot_frame(const ClipGeom& g, int slot) {
    const int64_t f = (int64_t)g.starts[slot >> 3] + (int64_t)(slot & 7) * g.f_skip;
    return f < g.F ? f : -1;
}

// The frame of `slot`, by the blocks blockIdx.x, blockIdx.x + bpf, ... of a frame: the groups of four of detect_frames_views_kernel over the
// H x W frame of g, merged logits into pl 16 bytes at a time, each logit fetched once, the views that cover each pixel as packed bytes into
// cv if it is not null.  pl and cv hold plane_stride floats / bytes: the padding of the last group takes merge_group4's values for pixels
// that do not exist (0.0f, cover 0); nothing reads it.
__device__ __forceinline__ void merge_to_plane(const ClipGeom& g, const float* logits, int slot, int bpf, float* pl, uint8_t* cv) {
    const uint32_t HW = (uint32_t)g.H * (uint32_t)g.W, total4 = (HW + 3u) >> 2;
    const size_t per = (size_t)g.S * g.S;
    const float* lp = logits + (size_t)slot * per;                   // view v: + v * view_stride * 8 * per
    const size_t vstep = (size_t)g.view_stride * 8 * per;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)bpf * BT) {
        const uint32_t px = idx << 2;
        float mg[4];
        int num[4], gy, gx;
        merge_group4(g, lp, vstep, px, HW, gy, gx, mg, num);
        f32x4 q;
        q[0] = mg[0]; q[1] = mg[1]; q[2] = mg[2]; q[3] = mg[3];
        *(f32x4*)(pl + px) = q;
        if (cv) *(uint32_t*)(cv + px) = (uint32_t)num[0] | ((uint32_t)num[1] << 8) | ((uint32_t)num[2] << 16) | ((uint32_t)num[3] << 24);
    }
}

// One tap row of the bilinear rule: the value at column pair (ix, ix + 1) of plane row r with the second weight wx1; `ok` is cleared when a
// tap that is read has no cover.  A tap of zero weight is not read.  Tap: a plane reader, float at(size_t idx) const.
template <class Tap>
__device__ __forceinline__ float tap_row(const Tap& tap, const uint8_t* cv, size_t r, int ix, int ix1, float wx0, float wx1, bool& ok) {
    const float a = tap.at(r + ix);
    ok = ok && cv[r + ix] != 0;
    if (wx1 == 0.0f) return a;
    const float b = tap.at(r + ix1);
    ok = ok && cv[r + ix1] != 0;
    return __fadd_rn(__fmul_rn(a, wx0), __fmul_rn(b, wx1));
}

// Native frame f of H x W, by the blocks blockIdx.x, blockIdx.x + bpf, ... (bpf = det_views_bpf(H * W)), in groups of four consecutive
// pixels (frame order, a group may run over a row's end): up to four taps of the Hs x Ws plane behind `tap` per pixel (tab:
// pc_resample_tables' rows [H][2], then columns [W][2]), every product and sum one fp32 round-to-nearest operation; then seg_positive, mask,
// box, score and the uint16 probability -- mask and prob [F][H][W] or null -- and the block's Partial to `out`.  The grouping depends on H, W
// alone, so the order of the sums is the same with any mask or prob or none.  The table's indices are clamped into the plane: a table that
// is not pc_resample_tables' for these sizes gives wrong values, never an access outside the plane.  Holds a block barrier.
template <class Tap>
__device__ __forceinline__ void detect_native_frame(const Tap& tap, const uint8_t* cv, const int32_t* tab, int64_t f, int H, int W, int Hs, int Ws,
                                                    uint8_t* mask, uint16_t* prob, int bpf, Partial* out) {
    const uint32_t HW = (uint32_t)H * (uint32_t)W, total4 = (HW + 3u) >> 2;
    const int32_t* rowt = tab;
    const int32_t* colt = tab + 2 * (size_t)H;
    uint8_t* mf = mask ? mask + (size_t)f * HW : nullptr;
    uint16_t* pf = prob ? prob + (size_t)f * HW : nullptr;
    FrameAcc acc;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)bpf * BT) {
        const uint32_t px = idx << 2;
        const int ny = (int)(HW - px < 4u ? HW - px : 4u);
        const int gy = (int)(px / (uint32_t)W), gx = (int)(px - (uint32_t)gy * (uint32_t)W);
        uint32_t bits = 0, q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= ny) continue;
            int y, x;
            group_pixel(gy, gx, e, W, y, x);
            const int iy = min(max(rowt[2 * y], 0), Hs - 1), iy1 = min(iy + 1, Hs - 1);
            const int ix = min(max(colt[2 * x], 0), Ws - 1), ix1 = min(ix + 1, Ws - 1);
            const float wy1 = __int_as_float(rowt[2 * y + 1]), wx1 = __int_as_float(colt[2 * x + 1]);
            const float wy0 = __fsub_rn(1.0f, wy1), wx0 = __fsub_rn(1.0f, wx1);
            bool ok = true;
            float v = tap_row(tap, cv, (size_t)iy * Ws, ix, ix1, wx0, wx1, ok);
            if (wy1 != 0.0f) {
                const float bot = tap_row(tap, cv, (size_t)iy1 * Ws, ix, ix1, wx0, wx1, ok);
                v = __fadd_rn(__fmul_rn(v, wy0), __fmul_rn(bot, wy1));
            }
            if (!ok) continue;                                       // a tap that was read has no cover: background, probability 0
            const float sg = sigmoid(v);
            q[e] = prob_word(v, sg);
            if (seg_positive(v)) {
                bits |= 1u << (8 * e);
                acc.add(sg, y, x);
            }
        }
        if (mf) store_mask4(mf + px, bits, ny);
        if (pf) store_prob4(pf + px, q, ny);
    }
    acc.block_partial(out);
}

// Words 0..4 of a record from a frame's accumulated share: the count and the half-open box, all zero for an empty frame.  (bx, by): what
// takes the box to full-frame coordinates.  True when the frame has a positive pixel.
__device__ __forceinline__ bool record_count_box(const FrameAcc& a, int bx, int by, int32_t* r) {
    const bool any = a.cnt > 0;
    r[0] = a.cnt;
    r[1] = any ? bx + a.x0 : 0; r[2] = any ? by + a.y0 : 0; r[3] = any ? bx + a.x1 + 1 : 0; r[4] = any ? by + a.y1 + 1 : 0;
    return any;
}

// A frame's block partials q[0 .. bpf) in block order, one division in double, one rounding to float -> the record r.  (bx, by): what takes
// the partials' box to full-frame coordinates; row: word 6, the frame's score row.
__device__ __forceinline__ void record_from_partials(const Partial* q, int bpf, int bx, int by, int row, int32_t* r) {
    FrameAcc a;
    for (int b = 0; b < bpf; ++b) a.add(q[b]);
    const bool any = record_count_box(a, bx, by, r);
    r[5] = __float_as_int(any ? (float)(a.sum / (double)a.cnt) : 0.0f);
    r[6] = row;
    r[7] = 0;
}

// one thread per (clip, frame of the clip).  (bx, by): the crop's corner for the centre traversal, (0, 0) for the views one, whose partials
// hold full-frame coordinates already; row_step: the score rows of one clip, so that the row is that of the clip's first view
__global__ __launch_bounds__(256) void detect_records_kernel(const DetectK p, int nframes, int bx, int by, int row_step) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= nframes) return;
    const int64_t f = slot_frame(p.g, t);
    if (f < 0) return;
    record_from_partials(p.part + (size_t)t * p.bpf, p.bpf, bx, by, p.row0 + (t >> 3) * row_step, p.rec + (size_t)f * REC_WORDS);
}

// blocks per frame: ~4 groups of four pixels per thread, at most 64.  A function of H * W alone.
inline int det_views_bpf(int64_t HW) {
    const int64_t n = ((HW + 3) / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

// floats of a merged plane, bytes of its cover: Hs * Ws rounded up to a multiple of four, so that a group's four floats and four cover
// bytes always go out as one 16-byte and one 4-byte store
inline size_t plane_stride(int Hs, int Ws) { return ((size_t)Hs * Ws + 3) & ~(size_t)3; }

// The checks pc_detect_frames, pc_detect_frames_views, pc_frame_probs and pc_detect_frames_scaled share, in the order they refuse; `who` names
// the entry in the messages.  crop: the (h0, w0) of the centre entry, which is the one view (h0, w0, 0) at stride n, or null for an entry that
// takes a view table.  The record entries write rec through ws from row0 on; pc_frame_probs (probs) writes prob alone and has none of the three.
inline int detect_args(ClipGeom& g, const char* who, const float* logits, int F, int H, int W, int S, const int32_t* crop, const int32_t* views,
                       int V, int view_stride, const int32_t* starts, int n, int f_skip, int row0, const void* rec, const void* ws, bool probs = false,
                       const void* prob = nullptr) {
    PC_CHECK_ARG(logits && views && starts && (probs ? prob != nullptr : rec && ws), "%s: null pointer", who);
    if (int rc = geom_shape(g, who, F, H, W, S, crop)) return rc;
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are outside the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(S % 4 == 0, "%s: S = %d must be a multiple of 4", who, S);
    if (int rc = geom_counts(g, who, V, n, view_stride, f_skip)) return rc;
    PC_CHECK_ARG(probs || (row0 >= 0 && row0 <= 0x7fffffff - MAX_CLIPS * (crop ? 1 : MAX_VIEWS)), "%s: row0 = %d", who, row0);
    PC_CHECK_ARG((uintptr_t)logits % 16 == 0, "%s: logits must be 16-byte aligned", who);
    PC_CHECK_ARG(probs || (((uintptr_t)ws % 8 == 0) && ((uintptr_t)rec % 4 == 0)), "%s: ws must be 8-byte and rec 4-byte aligned", who);
    PC_CHECK_ARG(!probs || (uintptr_t)prob % 2 == 0, "%s: prob must be 2-byte aligned", who);
    if (int rc = geom_views(g, who, views)) return rc;
    if (int rc = geom_starts(g, who, starts)) return rc;
    return PC_OK;
}

}  // namespace
