// What the detection entries of detect.hip (pc_detect_frames, pc_detect_frames_views, pc_frame_probs) and detectscale.hip
// (pc_detect_frames_scaled) share behind their traversal kernels, so that a record cannot mean two things:
//   Partial / DetectK       one block's share of a frame and the kernel arguments of the traversals and the records kernel
//   block_partial           a thread's share of a frame -> the block's Partial (thread -> wave -> block, a fixed order)
//   detect_records_kernel   the second launch: a frame's partials in block order -> its 8-word record
//   det_views_bpf           blocks per frame of a traversal over H * W pixels in groups of four
//   detect_args             the argument checks, in the order they refuse
// Everything here has internal linkage: each translation unit that includes it gets its own copy of the kernels.
#pragma once
#include "common.h"
#include "clipgeom.h"

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

// The end of the traversal kernels: a thread's share of a frame -> the block's Partial.  Count and box through the wave by shuffles, the
// four waves through LDS, thread 0 folds them in wave order.  Holds a block barrier: every thread of the block calls it.
__device__ __forceinline__ void block_partial(double sum, int cnt, int x0, int y0, int x1, int y1, Partial* out) {
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

// one thread per (clip, frame of the clip): the frame's block partials in block order, one division in double, one rounding to float.
// (bx, by): what takes the partials' box to full-frame coordinates -- the crop's corner for the centre traversal, (0, 0) for the views one,
// whose partials hold full-frame coordinates already; row_step: the score rows of one clip, so that the row is that of the clip's first view
__global__ __launch_bounds__(256) void detect_records_kernel(const DetectK p, int nframes, int bx, int by, int row_step) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= nframes) return;
    const int c = t >> 3, k = t & 7;
    const int64_t f = (int64_t)p.g.starts[c] + (int64_t)k * p.g.f_skip;
    if (f >= p.g.F) return;
    const Partial* q = p.part + (size_t)t * p.bpf;
    double sum = 0.0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (int b = 0; b < p.bpf; ++b) {
        sum += q[b].sum; cnt += q[b].count;
        x0 = min(x0, q[b].x0); y0 = min(y0, q[b].y0); x1 = max(x1, q[b].x1); y1 = max(y1, q[b].y1);
    }
    int32_t* r = p.rec + (size_t)f * REC_WORDS;
    const bool any = cnt > 0;
    r[0] = cnt;
    r[1] = any ? bx + x0 : 0; r[2] = any ? by + y0 : 0; r[3] = any ? bx + x1 + 1 : 0; r[4] = any ? by + y1 + 1 : 0;
    r[5] = __float_as_int(any ? (float)(sum / (double)cnt) : 0.0f);
    r[6] = p.row0 + c * row_step;
    r[7] = 0;
}

// blocks per frame: ~4 groups of four pixels per thread, at most 64.  A function of H * W alone.
inline int det_views_bpf(int64_t HW) {
    const int64_t n = ((HW + 3) / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

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
