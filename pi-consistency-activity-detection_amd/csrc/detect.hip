// Detection output on the device: what a caller of the eval forward had to do on the host to get from a batch of logits to "where is the
// action, and which one" -- sigmoid, threshold, a device-to-host copy of every mask, the bounding box in numpy and the undoing of the clip
// interleave (frame k of clip c is video frame starts[c] + k * f_skip) by hand.
//   pc_detect_frames   the inverse of pc_clips_from_u8's gather fused with the per-frame reductions: up to 32 clips of logits into the
//                      video-order uint8 masks (full frames, margin included) and one 8-word record per frame (count, box, score, row);
//                      HBM-bound, 4 bytes read per crop pixel and 1 written per frame pixel
//   pc_video_class     mean class scores, their arg-max and its score: pc_video_vote's reduction, returned instead of compared
//   pc_detect_frames_views   pc_detect_frames with the logits of V views merged per full-frame pixel in front of it (below)
//   pc_frame_probs     the per-pixel probability of the merged logit as uint16 in video order, for pc_instance_scores (end of this file);
//                      its merge is the views kernel's own (viewmerge.h: merge_group4's), no records, no workspace
// Two traversal kernels (detect_frames_kernel walks the crop's float4 and then the margin, detect_frames_views_kernel the full frame in
// groups of four: another memory traffic and another order of the sums), one accumulator and end (FrameAcc), one mask and one probability
// store, one probability conversion, one records kernel, one set of argument checks (detect_args) on the geometry of clipgeom.h -- all in
// detectrec.h, which detectscale.hip and cliphop.hip share.
// The mask predicate is the evaluator's own (evalpred.h: seg_positive, shared with pc_seg_frame_counts).  No floating-point atomics and no
// integer ones either: every block leaves one partial in a caller-owned workspace, a second small launch adds them in block order (the
// pattern of valmetrics.hip), so a record is bit-identical from run to run and nothing has to be zeroed in front of the launch.
#include "detectrec.h"

namespace {

// blocks per frame: ~4 float4 per thread, at most 64 (the block-stride loop covers the rest).  A function of S alone.
inline int det_bpf(int S) {
    const int64_t n = ((int64_t)S * S / 4 + BT * 4 - 1) / (BT * 4);
    return (int)(n < 1 ? 1 : (n > 64 ? 64 : n));
}

// grid (bpf, n * 8): blockIdx.y = clip * 8 + frame of the clip, the bpf blocks of a frame stride over its S*S/4 float4 of logits (a wave:
// 1 KiB contiguous) and then over the HW - S*S bytes of margin around the crop.  A thread's four mask bytes go out as one dword where the
// address allows (a mask row starts at any byte address when W is odd), as four bytes otherwise.
__global__ __launch_bounds__(256) void detect_frames_kernel(const DetectK p) {
    const ClipGeom& g = p.g;
    const int64_t f = slot_frame(g, blockIdx.y);
    if (f < 0) return;
    const int S = g.S, S4 = S >> 2, total4 = S * S4, H = g.H, W = g.W, h0 = g.vh0[0], w0 = g.vw0[0];
    const f32x4* lp = (const f32x4*)p.logits + (size_t)blockIdx.y * total4;
    uint8_t* mf = p.mask ? p.mask + (size_t)f * H * W : nullptr;
    FrameAcc acc;
    for (int idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += p.bpf * BT) {
        const int y = idx / S4, x = (idx - y * S4) << 2;
        const f32x4 v = lp[idx];
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (seg_positive(v[e])) {
                bits |= 1u << (8 * e);
                acc.add(sigmoid(v[e]), y, x + e);
            }
        }
        if (mf) store_mask4(mf + (size_t)(h0 + y) * W + w0 + x, bits, 4);
    }
    if (mf) {
        // the margin as S + 1 runs of bytes: the rows above the crop and the first row's left margin, the W - S bytes between the crop rows,
        // the last row's right margin and the rows below
        const int gap = W - S;
        const int head = h0 * W + w0, mid = (S - 1) * gap, margin = H * W - S * S;
        const int tail0 = (h0 + S - 1) * W + w0 + S;
        for (int m = blockIdx.x * BT + threadIdx.x; m < margin; m += p.bpf * BT) {
            int a;
            if (m < head) a = m;
            else if (m - head < mid) { const int y = (m - head) / gap, j = (m - head) - y * gap; a = (h0 + y) * W + w0 + S + j; }
            else a = tail0 + (m - head - mid);
            mf[a] = 0;
        }
    }
    acc.block_partial(p.part + (size_t)blockIdx.y * p.bpf + blockIdx.x);
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
    const int32_t view[3] = {h0, w0, 0};
    DetectK k;
    if (int rc = detect_args(k.g, "pc_detect_frames", logits, F, H, W, S, view, view, 1, n, starts, n, f_skip, row0, rec, ws)) return rc;
    k.logits = logits; k.mask = mask; k.rec = rec; k.part = (Partial*)ws; k.row0 = row0;
    k.bpf = det_bpf(S);
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(detect_frames_kernel, dim3((unsigned)k.bpf, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(detect_records_kernel, dim3((unsigned)cdiv(n * 8, BT)), dim3(BT), 0, s, k, n * 8, w0, h0, 1);
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

// grid (bpf, n * 8): blockIdx.y = clip * 8 + frame of the clip; the bpf blocks of a frame stride over its H*W pixels in groups of four
// consecutive ones (frame order, a group may run over a row's end).  Where a group lies in one row and a view covers all of it from a
// 16-byte boundary of its logit row, the view's four values come as one float4 (backwards for a mirrored view); otherwise one by one.  The
// grouping depends on H, W alone -- not on where the mask lies -- so the order of the sums, and with it a record, is the same with any mask
// or none; the four mask bytes go out as one dword where their address allows, as bytes otherwise.
__global__ __launch_bounds__(256) void detect_frames_views_kernel(const DetectK p) {
    const ClipGeom& g = p.g;
    const int64_t f = slot_frame(g, blockIdx.y);
    if (f < 0) return;
    const uint32_t HW = (uint32_t)g.H * (uint32_t)g.W, total4 = (HW + 3u) >> 2;
    const size_t per = (size_t)g.S * g.S;
    const float* lp = p.logits + (size_t)blockIdx.y * per;           // view v: + v * view_stride * 8 * per
    const size_t vstep = (size_t)g.view_stride * 8 * per;
    uint8_t* mf = p.mask ? p.mask + (size_t)f * HW : nullptr;
    FrameAcc acc;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)p.bpf * BT) {
        const uint32_t px = idx << 2;
        float mg[4];
        int num[4], gy, gx;
        const int ny = merge_group4(g, lp, vstep, px, HW, gy, gx, mg, num);
        uint32_t bits = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (num[e] == 0 || !seg_positive(mg[e])) continue;       // no view covers the pixel, or its merged logit fails the predicate: background
            int y, x;
            group_pixel(gy, gx, e, g.W, y, x);
            bits |= 1u << (8 * e);
            acc.add(sigmoid(mg[e]), y, x);
        }
        if (mf) store_mask4(mf + px, bits, ny);
    }
    acc.block_partial(p.part + (size_t)blockIdx.y * p.bpf + blockIdx.x);
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
    DetectK k;
    if (int rc = detect_args(k.g, who, logits, F, H, W, S, nullptr, views, V, view_stride, starts, n, f_skip, row0, rec, ws)) return rc;
    k.logits = logits; k.mask = mask; k.rec = rec; k.part = (Partial*)ws; k.row0 = row0;
    k.bpf = det_views_bpf((int64_t)H * W);
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(detect_frames_views_kernel, dim3((unsigned)k.bpf, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(detect_records_kernel, dim3((unsigned)cdiv(n * 8, BT)), dim3(BT), 0, s, k, n * 8, 0, 0, V);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

// ---------------------------------------------------------------------- the probability map (detect.DetectEngine, instance_scores)
//   pc_frame_probs   the per-pixel probability of the merged logit in video order: what the frame score sums, kept as uint16 so that
//                    pc_instance_scores (instances.hip) can reduce it per instance behind the video's last clip.  The merged logit is
//                    merge_group4's, the one the mask was thresholded on.  Reads logits the detect launch in front of it has just read
//                    (cache-resident), writes 2 bytes per frame pixel.  No atomics, no LDS, no workspace.
namespace {

struct ProbK {
    const float* logits; uint16_t* prob;
    int bpf;
    ClipGeom g;
};

// grid (bpf, n * 8) and the groups of four of detect_frames_views_kernel.  A group's four values go out as one 8-byte store where the address
// allows (a frame of odd H * W starts at an odd element), as 2-byte stores otherwise; a group that crosses the frame's end writes its ny.
__global__ __launch_bounds__(256) void frame_probs_kernel(const ProbK p) {
    const ClipGeom& g = p.g;
    const int64_t f = slot_frame(g, blockIdx.y);
    if (f < 0) return;
    const uint32_t HW = (uint32_t)g.H * (uint32_t)g.W, total4 = (HW + 3u) >> 2;
    const size_t per = (size_t)g.S * g.S;
    const float* lp = p.logits + (size_t)blockIdx.y * per;           // view v: + v * view_stride * 8 * per
    const size_t vstep = (size_t)g.view_stride * 8 * per;
    uint16_t* pf = p.prob + (size_t)f * HW;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)p.bpf * BT) {
        const uint32_t px = idx << 2;
        float mg[4];
        int num[4], gy, gx;
        const int ny = merge_group4(g, lp, vstep, px, HW, gy, gx, mg, num);
        uint32_t q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = num[e] ? prob_word(mg[e], sigmoid(mg[e])) : 0u;     // no view covers the pixel: 0
        store_prob4(pf + px, q, ny);
    }
}

}  // namespace

extern "C" int pc_frame_probs(const float* logits, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                              const int32_t* starts, int n, int f_skip, uint16_t* prob, pc_stream s) {
    const char* who = "pc_frame_probs";
    ProbK k;
    if (int rc = detect_args(k.g, who, logits, F, H, W, S, nullptr, views, V, view_stride, starts, n, f_skip, 0, nullptr, nullptr, true, prob)) return rc;
    k.logits = logits; k.prob = prob;
    k.bpf = det_views_bpf((int64_t)H * W);
    hipLaunchKernelGGL(frame_probs_kernel, dim3((unsigned)k.bpf, (unsigned)(n * 8)), dim3(BT), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
