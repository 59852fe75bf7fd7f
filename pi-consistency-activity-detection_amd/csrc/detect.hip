// Detection output on the device: what a caller of the eval forward had to do on the host to get from a batch of logits to "where is the
// action, and which one" -- sigmoid, threshold, a device-to-host copy of every mask, the bounding box in numpy and the undoing of the clip
// interleave (frame k of clip c is video frame starts[c] + k * f_skip) by hand.
//   pc_detect_frames   the inverse of pc_clips_from_u8's gather fused with the per-frame reductions: up to 32 clips of logits into the
//                      video-order uint8 masks (full frames, margin included) and one 8-word record per frame (count, box, score, row);
//                      HBM-bound, 4 bytes read per crop pixel and 1 written per frame pixel
//   pc_video_class     mean class scores, their arg-max and its score: pc_video_vote's reduction, returned instead of compared
//   pc_detect_frames_views   pc_detect_frames with the logits of V views merged per full-frame pixel in front of it (end of this file)
// The mask predicate is the evaluator's own (evalpred.h: seg_positive, shared with pc_seg_frame_counts).  No floating-point atomics and no
// integer ones either: every block leaves one partial in a caller-owned workspace, a second small launch adds them in block order (the
// pattern of valmetrics.hip), so a record is bit-identical from run to run and nothing has to be zeroed in front of the launch.
#include "common.h"
#include "evalpred.h"

namespace {

constexpr int MAX_CLIPS = 32;
constexpr int BT = 256, NW = BT / 64;
constexpr int REC_WORDS = 8;

struct Partial {                 // one block's share of a frame, crop coordinates; 32 bytes
    double sum;                  // sum of sigmoid(x) over its positive pixels, in the fixed order thread -> wave -> block
    int32_t count, x0, y0, x1, y1, pad;      // closed box; count == 0: the box is (INT_MAX, INT_MAX, -1, -1)
};

// blocks per frame: ~4 float4 per thread, at most 64 (the block-stride loop covers the rest).  A function of S alone.
inline int det_bpf(int S) {
    const int64_t n = ((int64_t)S * S / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

struct DetectK {
    const f32x4* logits; uint8_t* mask; int32_t* rec; Partial* part;
    int F, H, W, h0, w0, S, f_skip, row0, bpf;
    int starts[MAX_CLIPS];
};

// grid (bpf, n * 8): blockIdx.y = clip * 8 + frame of the clip, the bpf blocks of a frame stride over its S*S/4 float4 of logits (a wave:
// 1 KiB contiguous) and then over the HW - S*S bytes of margin around the crop.  A thread's four mask bytes go out as one dword where the
// address allows (a mask row starts at any byte address when W is odd), as four bytes otherwise.
__global__ __launch_bounds__(256) void detect_frames_kernel(const DetectK p) {
    __shared__ double shs[NW];
    __shared__ int shi[NW][5];
    const int c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    if (f >= p.F) return;                                            // a frame past the end: nothing read, nothing written
    const int S = p.S, S4 = S >> 2, total4 = S * S4;
    const f32x4* lp = p.logits + (size_t)blockIdx.y * total4;
    uint8_t* mf = p.mask ? p.mask + (size_t)f * p.H * p.W : nullptr;
    double sum = 0.0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (int idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += p.bpf * BT) {
        const int y = idx / S4, x = (idx - y * S4) << 2;
        const f32x4 v = lp[idx];
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (seg_positive(v[e])) {
                bits |= 1u << (8 * e);
                sum += (double)(1.0f / (1.0f + expf(-v[e])));
                ++cnt;
                x0 = min(x0, x + e); x1 = max(x1, x + e);
            }
        }
        if (bits) { y0 = min(y0, y); y1 = max(y1, y); }
        if (mf) {
            uint8_t* m = mf + (size_t)(p.h0 + y) * p.W + p.w0 + x;
            if (((uintptr_t)m & 3) == 0) {
                *(uint32_t*)m = bits;
            } else {
                m[0] = (uint8_t)(bits & 1); m[1] = (uint8_t)((bits >> 8) & 1); m[2] = (uint8_t)((bits >> 16) & 1); m[3] = (uint8_t)(bits >> 24);
            }
        }
    }
    if (mf) {
        // the margin as S + 1 runs of bytes: the rows above the crop and the first row's left margin, the W - S bytes between the crop rows,
        // the last row's right margin and the rows below
        const int gap = p.W - S;
        const int head = p.h0 * p.W + p.w0, mid = (S - 1) * gap, margin = p.H * p.W - S * S;
        const int tail0 = (p.h0 + S - 1) * p.W + p.w0 + S;
        for (int m = blockIdx.x * BT + threadIdx.x; m < margin; m += p.bpf * BT) {
            int a;
            if (m < head) a = m;
            else if (m - head < mid) { const int y = (m - head) / gap, j = (m - head) - y * gap; a = (p.h0 + y) * p.W + p.w0 + S + j; }
            else a = tail0 + (m - head - mid);
            mf[a] = 0;
        }
    }
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
        p.part[(size_t)blockIdx.y * p.bpf + blockIdx.x] = q;
    }
}

// one thread per (clip, frame of the clip): the frame's block partials in block order, one division in double, one rounding to float
__global__ __launch_bounds__(256) void detect_records_kernel(const DetectK p, int nframes) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= nframes) return;
    const int c = t >> 3, k = t & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    if (f >= p.F) return;
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
    r[1] = any ? p.w0 + x0 : 0; r[2] = any ? p.h0 + y0 : 0; r[3] = any ? p.w0 + x1 + 1 : 0; r[4] = any ? p.h0 + y1 + 1 : 0;
    r[5] = __float_as_int(any ? (float)(sum / (double)cnt) : 0.0f);
    r[6] = p.row0 + c;
    r[7] = 0;
}

__global__ __launch_bounds__(256) void video_class_kernel(const float* __restrict__ scores, int n, int C, float* __restrict__ out) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    float best; int besti;
    vote_mean_argmax(scores, n, C, out, bv, bi, best, besti);
    if (threadIdx.x == 0) { out[C] = (float)besti; out[C + 1] = best; }
}

inline bool det_shape_ok(int n, int S) { return n >= 1 && n <= MAX_CLIPS && S >= 4 && S <= 32768 && S % 4 == 0; }

}  // namespace

extern "C" int64_t pc_detect_frames_ws_bytes(int n, int S) {
    if (!det_shape_ok(n, S)) return -1;
    return (int64_t)n * 8 * det_bpf(S) * (int64_t)sizeof(Partial);
}

extern "C" int pc_detect_frames(const float* logits, int F, int H, int W, int h0, int w0, int S, const int32_t* starts, int n, int f_skip,
                                int row0, uint8_t* mask, int32_t* rec, void* ws, pc_stream s_) {
    PC_CHECK_ARG(logits && starts && rec && ws, "pc_detect_frames: null pointer");
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768 && h0 >= 0 && w0 >= 0 && (int64_t)h0 + S <= H && (int64_t)w0 + S <= W,
                 "pc_detect_frames: %d frames, crop %d+%d x %d+%d outside %d x %d", F, h0, S, w0, S, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "pc_detect_frames: frames of %d x %d pixels are outside the 2^31 a frame may hold", H, W);
    PC_CHECK_ARG(S % 4 == 0, "pc_detect_frames: S = %d must be a multiple of 4", S);
    PC_CHECK_ARG(n >= 1 && n <= MAX_CLIPS, "pc_detect_frames: n = %d clips outside 1..%d", n, MAX_CLIPS);
    PC_CHECK_ARG(f_skip >= 1, "pc_detect_frames: f_skip = %d", f_skip);
    PC_CHECK_ARG(row0 >= 0 && row0 <= 0x7fffffff - MAX_CLIPS, "pc_detect_frames: row0 = %d", row0);
    PC_CHECK_ARG((uintptr_t)logits % 16 == 0, "pc_detect_frames: logits must be 16-byte aligned");
    PC_CHECK_ARG(((uintptr_t)ws % 8 == 0) && ((uintptr_t)rec % 4 == 0), "pc_detect_frames: ws must be 8-byte and rec 4-byte aligned");
    DetectK k;
    k.logits = (const f32x4*)logits; k.mask = mask; k.rec = rec; k.part = (Partial*)ws;
    k.F = F; k.H = H; k.W = W; k.h0 = h0; k.w0 = w0; k.S = S; k.f_skip = f_skip; k.row0 = row0; k.bpf = det_bpf(S);
    for (int c = 0; c < MAX_CLIPS; ++c) {
        if (c < n) PC_CHECK_ARG(starts[c] >= 0, "pc_detect_frames: start %d of clip %d is negative", starts[c], c);
        k.starts[c] = c < n ? starts[c] : 0;
    }
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(detect_frames_kernel, dim3((unsigned)k.bpf, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(detect_records_kernel, dim3((unsigned)cdiv(n * 8, BT)), dim3(BT), 0, s, k, n * 8);
    PC_CHECK_LAUNCH("detect_frames");
    return PC_OK;
}

extern "C" int pc_video_class(const float* scores, int n, int C, float* out, pc_stream s) {
    PC_CHECK_ARG(scores && out, "pc_video_class: null pointer");
    PC_CHECK_ARG(n >= 1 && C >= 1 && (int64_t)n * C < (1ll << 31), "pc_video_class: n = %d rows of C = %d scores", n, C);
    hipLaunchKernelGGL(video_class_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, scores, n, C, out);
    PC_CHECK_LAUNCH("video_class");
    return PC_OK;
}

// ---------------------------------------------------------------------- views (detect.DetectEngine, tile / flip)
//   pc_detect_frames_views   pc_detect_frames for V views of every clip (crops at their own offsets, some mirrored): per FULL-FRAME pixel the
//                            logits of the views that cover it, in table order, become one merged logit (the first as it is, the others
//                            added with __fadd_rn, one __fdiv_rn by the count when more than one covers) in front of the predicate, the box
//                            and the score; a pixel no view covers is background.  HBM-bound, 4 bytes read per view pixel and 1 written per
//                            frame pixel.  Same partials, same second launch, same records.
namespace {

constexpr int MAX_VIEWS = 32;

// blocks per frame: ~4 groups of four pixels per thread, at most 64.  A function of H * W alone.
inline int det_views_bpf(int64_t HW) {
    const int64_t n = ((HW + 3) / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

struct DetectViewsK {
    const float* logits; uint8_t* mask; int32_t* rec; Partial* part;
    int F, H, W, S, f_skip, row0, bpf, V, view_stride;
    int starts[MAX_CLIPS];
    int vh0[MAX_VIEWS], vw0[MAX_VIEWS];
    uint32_t flips;                                                  // bit v: view v is mirrored left-right
};

// grid (bpf, n * 8): blockIdx.y = clip * 8 + frame of the clip; the bpf blocks of a frame stride over its H*W pixels in groups of four
// consecutive ones (frame order, a group may run over a row's end).  Where a group lies in one row and a view covers all of it from a
// 16-byte boundary of its logit row, the view's four values come as one float4 (backwards for a mirrored view); otherwise one by one.  The
// grouping depends on H, W alone -- not on where the mask lies -- so the order of the sums, and with it a record, is the same with any mask
// or none; the four mask bytes go out as one dword where their address allows, as bytes otherwise.
__global__ __launch_bounds__(256) void detect_frames_views_kernel(const DetectViewsK p) {
    __shared__ double shs[NW];
    __shared__ int shi[NW][5];
    const int c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    if (f >= p.F) return;                                            // a frame past the end: nothing read, nothing written
    const int S = p.S, W = p.W;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)W, total4 = (HW + 3u) >> 2;
    const size_t per = (size_t)S * S;
    const float* lp = p.logits + ((size_t)c * 8 + k) * per;          // view v: + v * view_stride * 8 * per
    const size_t vstep = (size_t)p.view_stride * 8 * per;
    uint8_t* mf = p.mask ? p.mask + (size_t)f * HW : nullptr;
    double sum = 0.0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)p.bpf * BT) {
        const uint32_t px = idx << 2;
        const int ny = (int)(HW - px < 4u ? HW - px : 4u);           // pixels of the group inside the frame
        const int gy = (int)(px / (uint32_t)W), gx = (int)(px - (uint32_t)gy * (uint32_t)W);
        const bool row = ny == 4 && gx + 3 < W;                      // the group lies in one row
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int num[4] = {0, 0, 0, 0};
        for (int v = 0; v < p.V; ++v) {
            const int h0 = p.vh0[v], w0 = p.vw0[v];
            const bool flip = (p.flips >> v) & 1u;
            const float* lv = lp + (size_t)v * vstep;
            const int dy = gy - h0, dx = gx - w0;
            if (row && dy >= 0 && dy < S && dx >= 0 && dx + 3 < S && (dx & 3) == 0) {
                const f32x4 q = *(const f32x4*)(lv + (size_t)dy * S + (flip ? S - 4 - dx : dx));
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = flip ? q[3 - e] : q[e];
                    acc[e] = num[e] ? __fadd_rn(acc[e], t) : t;
                    ++num[e];
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                int y = gy, x = gx + e;
                if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; } } }     // W >= 1: at most three rows on
                const int ey = y - h0, ex = x - w0;
                if (e < ny && ey >= 0 && ey < S && ex >= 0 && ex < S) {
                    const float t = lv[(size_t)ey * S + (flip ? S - 1 - ex : ex)];
                    acc[e] = num[e] ? __fadd_rn(acc[e], t) : t;
                    ++num[e];
                }
            }
        }
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (num[e] == 0) continue;                               // no view covers the pixel: background
            const float m = num[e] > 1 ? __fdiv_rn(acc[e], (float)num[e]) : acc[e];
            if (seg_positive(m)) {
                int y = gy, x = gx + e;
                if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; } } }
                bits |= 1u << (8 * e);
                sum += (double)(1.0f / (1.0f + expf(-m)));
                ++cnt;
                x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
            }
        }
        if (mf) {
            uint8_t* m = mf + px;
            if (ny == 4 && ((uintptr_t)m & 3) == 0) {
                *(uint32_t*)m = bits;
            } else {
                for (int e = 0; e < ny; ++e) m[e] = (uint8_t)((bits >> (8 * e)) & 1);
            }
        }
    }
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
        p.part[(size_t)blockIdx.y * p.bpf + blockIdx.x] = q;
    }
}

// one thread per (clip, frame of the clip), as detect_records_kernel: the partials hold full-frame coordinates already, and the row is that
// of the clip's first view
__global__ __launch_bounds__(256) void detect_views_records_kernel(const DetectViewsK p, int nframes) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= nframes) return;
    const int c = t >> 3, k = t & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    if (f >= p.F) return;
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
    r[1] = any ? x0 : 0; r[2] = any ? y0 : 0; r[3] = any ? x1 + 1 : 0; r[4] = any ? y1 + 1 : 0;
    r[5] = __float_as_int(any ? (float)(sum / (double)cnt) : 0.0f);
    r[6] = p.row0 + c * p.V;
    r[7] = 0;
}

inline bool det_views_shape_ok(int n, int H, int W) { return n >= 1 && n <= MAX_CLIPS && H >= 1 && W >= 1 && (int64_t)H * W < (1ll << 31); }

}  // namespace

extern "C" int64_t pc_detect_frames_views_ws_bytes(int n, int H, int W) {
    if (!det_views_shape_ok(n, H, W)) return -1;
    return (int64_t)n * 8 * det_views_bpf((int64_t)H * W) * (int64_t)sizeof(Partial);
}

extern "C" int pc_detect_frames_views(const float* logits, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                                      const int32_t* starts, int n, int f_skip, int row0, uint8_t* mask, int32_t* rec, void* ws, pc_stream s_) {
    const char* who = "pc_detect_frames_views";
    PC_CHECK_ARG(logits && views && starts && rec && ws, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768 && S <= H && S <= W, "%s: %d frames, crop of %d outside %d x %d", who, F, S, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are outside the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(S % 4 == 0, "%s: S = %d must be a multiple of 4", who, S);
    PC_CHECK_ARG(V >= 1 && V <= MAX_VIEWS, "%s: V = %d views outside 1..%d", who, V, MAX_VIEWS);
    PC_CHECK_ARG(n >= 1 && n <= MAX_CLIPS, "%s: n = %d clips outside 1..%d", who, n, MAX_CLIPS);
    PC_CHECK_ARG(view_stride >= n, "%s: view_stride = %d is below the n = %d clips of a view", who, view_stride, n);
    PC_CHECK_ARG(f_skip >= 1, "%s: f_skip = %d", who, f_skip);
    PC_CHECK_ARG(row0 >= 0 && row0 <= 0x7fffffff - MAX_CLIPS * MAX_VIEWS, "%s: row0 = %d", who, row0);
    PC_CHECK_ARG((uintptr_t)logits % 16 == 0, "%s: logits must be 16-byte aligned", who);
    PC_CHECK_ARG(((uintptr_t)ws % 8 == 0) && ((uintptr_t)rec % 4 == 0), "%s: ws must be 8-byte and rec 4-byte aligned", who);
    DetectViewsK k;
    k.logits = logits; k.mask = mask; k.rec = rec; k.part = (Partial*)ws;
    k.F = F; k.H = H; k.W = W; k.S = S; k.f_skip = f_skip; k.row0 = row0; k.bpf = det_views_bpf((int64_t)H * W); k.V = V; k.view_stride = view_stride;
    k.flips = 0;
    for (int v = 0; v < MAX_VIEWS; ++v) {
        k.vh0[v] = k.vw0[v] = 0;
        if (v >= V) continue;
        const int h0 = views[3 * v], w0 = views[3 * v + 1], fl = views[3 * v + 2];
        PC_CHECK_ARG(h0 >= 0 && w0 >= 0 && (int64_t)h0 + S <= H && (int64_t)w0 + S <= W, "%s: view %d, crop %d+%d x %d+%d outside %d x %d", who, v,
                     h0, S, w0, S, H, W);
        PC_CHECK_ARG(fl == 0 || fl == 1, "%s: view %d, flip = %d is neither 0 nor 1", who, v, fl);
        k.vh0[v] = h0; k.vw0[v] = w0; k.flips |= (uint32_t)fl << v;
    }
    for (int c = 0; c < MAX_CLIPS; ++c) {
        if (c < n) PC_CHECK_ARG(starts[c] >= 0, "%s: start %d of clip %d is negative", who, starts[c], c);
        k.starts[c] = c < n ? starts[c] : 0;
    }
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(detect_frames_views_kernel, dim3((unsigned)k.bpf, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(detect_views_records_kernel, dim3((unsigned)cdiv(n * 8, BT)), dim3(BT), 0, s, k, n * 8);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
