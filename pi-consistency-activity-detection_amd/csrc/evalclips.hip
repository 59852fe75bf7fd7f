// Evaluation input on the device: what the reference's eval loop does per video on the host before the network sees a clip
// (evaluate_ucf101.py:79-101 on the centre-cropped frames and truth of datasets/ucf_dataloader_eval.py:100-106) and the class vote
// behind it (:139-146), from the decoded uint8 frames and uint8 truth already in HBM.
//   pc_truth_frame_flags   per frame, the number of non-zero truth pixels inside the crop: decides which clips are kept (:95-96)
//   pc_eval_clips_from_u8  up to 32 clips of one video straight into the NDHWC tensor the stem reads and the frame-major truth
//                          pc_seg_frame_counts takes; HBM-bound, 4 bytes read and 20 written per pixel
//   pc_clips_from_u8       the same kernel without the truth side (unlabelled video: picons_amd/detect.py)
//   pc_clips_from_u8_views pc_clips_from_u8 for V views (crops at their own offsets, some mirrored left-right) of the clips in one launch
//                          all three are clips_from_u8_kernel<TRUTH> on the geometry of clipgeom.h: a centre crop is one view at stride n
//   pc_video_vote          argmax(mean(predictions, axis=0)) == label, rows added in order in fp32 as numpy adds them
#include "common.h"
#include "evalpred.h"
#include "clipgeom.h"

namespace {

__global__ __launch_bounds__(256) void truth_frame_flags_kernel(const uint8_t* __restrict__ truth, int H, int W, int h0, int w0, int S,
                                                                int32_t* __restrict__ flags) {
    __shared__ int part[4];
    const uint8_t* fr = truth + ((size_t)blockIdx.x * H + h0) * W + w0;
    const int total = S * S;
    int cnt = 0;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int y = idx / S, x = idx - y * S;
        cnt += fr[(size_t)y * W + x] != 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

struct ClipCutK {
    const uint8_t* video; const uint8_t* truth;
    float4* data; float* gt;
    ClipGeom g;
};

// One frame of one view: FLIP reads the row backwards.  A template, and one branch per block, so that the unmirrored loop -- all there is to
// the centre entries -- carries nothing of the mirror.  Selecting the column per pixel, and the view as blockIdx.y / (n * 8), put the centre
// entries 2 - 3 % above the parent's kernel time (docs/MEASUREMENTS.md, "One clip cut": builds, shapes and every figure).
template <bool TRUTH, bool FLIP>
__device__ __forceinline__ void cut_frame(const float* lut, const uint8_t* vf, const uint8_t* tf, int S, int W, float4* data, float* gt) {
    const int total = S * S;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / S, x = idx - y * S;
        const size_t src = (size_t)y * W + (FLIP ? S - 1 - x : x);
        const uint8_t* px = vf + src * 3;
        data[idx] = make_float4(lut[px[0]], lut[px[1]], lut[px[2]], 0.f);
        if (TRUTH) gt[idx] = (float)tf[src];                         // the value itself: the reference counts pred + gt == 2
    }
}

// blockIdx.z = view, blockIdx.y = clip * 8 + frame of the clip, written at clip slot view * view_stride + clip; blockIdx.x strides over the frame's
// S*S pixels: one thread per pixel writes one whole float4 (a wave: 1 KiB contiguous) and one truth float (256 B contiguous).  The source
// bytes of a cropped RGB row start at any byte address, so they are read as bytes; consecutive lanes read consecutive 3-byte pixels of one
// row, descending ones for a mirrored view, which reads its row backwards.
// TRUTH = false (pc_clips_from_u8, pc_clips_from_u8_views): the same body without the truth side; p.truth and p.gt are never touched.
template <bool TRUTH>
__global__ __launch_bounds__(256) void clips_from_u8_kernel(const ClipCutK p) {
    __shared__ float lut[256];
    const ClipGeom& g = p.g;
    const int v = blockIdx.z, c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)g.starts[c] + (int64_t)k * g.f_skip;
    const int vh0 = g.vh0[v], vw0 = g.vw0[v];                        // the block's table entries: asked for in front of the division below
    const bool flip = (g.flips >> v) & 1u;
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);        // img / 255. in float64, then the float32 cast: once per block
    __syncthreads();
    const int S = g.S, total = S * S;
    const size_t at = (((size_t)v * g.view_stride + c) * 8 + k) * total;
    float4* data = p.data + at;
    float* gt = TRUTH ? p.gt + at : nullptr;
    if (f >= g.F) {                                                  // a frame past the end: zeros, nothing read (evaluate_ucf101.py:89-91)
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
            data[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (TRUTH) gt[idx] = 0.f;
        }
        return;
    }
    const size_t corner = ((size_t)f * g.H + vh0) * g.W + vw0;
    const uint8_t* vf = p.video + corner * 3;
    const uint8_t* tf = TRUTH ? p.truth + corner : nullptr;
    if (flip) cut_frame<TRUTH, true>(lut, vf, tf, S, g.W, data, gt);
    else cut_frame<TRUTH, false>(lut, vf, tf, S, g.W, data, gt);
}

__global__ __launch_bounds__(256) void video_vote_kernel(const float* __restrict__ pred, int n, int C, int label, int32_t* n_correct) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    float best; int besti;
    vote_mean_argmax(pred, n, C, nullptr, bv, bi, best, besti);     // evalpred.h: the reduction pc_video_class shares
    if (threadIdx.x == 0 && besti == label) *n_correct += 1;
}

}  // namespace

extern "C" int pc_truth_frame_flags(const uint8_t* truth, int F, int H, int W, int h0, int w0, int S, int32_t* flags, pc_stream s) {
    PC_CHECK_ARG(truth && flags, "pc_truth_frame_flags: null pointer");
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768 && h0 >= 0 && w0 >= 0 && (int64_t)h0 + S <= H && (int64_t)w0 + S <= W,
                 "pc_truth_frame_flags: %d frames, crop %d+%d x %d+%d outside %d x %d", F, h0, S, w0, S, H, W);
    hipLaunchKernelGGL(truth_frame_flags_kernel, dim3((unsigned)F), dim3(256), 0, (hipStream_t)s, truth, H, W, h0, w0, S, flags);
    PC_CHECK_LAUNCH("truth_frame_flags");
    return PC_OK;
}

// The checks and the launch of the three cut entries; `who` names the entry in the messages.  crop: the (h0, w0) of a centre-crop entry, which
// is the one view (h0, w0, 0) at stride n, or null for the entry that takes a view table.
template <bool TRUTH>
static int clips_from_u8(const char* who, const uint8_t* video, const uint8_t* truth, int F, int H, int W, int S, const int32_t* crop,
                         const int32_t* views, int V, int view_stride, const int32_t* starts, int n, int f_skip, float* data, float* gt,
                         pc_stream s) {
    ClipCutK k;
    PC_CHECK_ARG(video && views && starts && data && (!TRUTH || (truth && gt)), "%s: null pointer", who);
    if (int rc = geom_shape(k.g, who, F, H, W, S, crop)) return rc;
    if (int rc = geom_counts(k.g, who, V, n, view_stride, f_skip)) return rc;
    PC_CHECK_ARG(((uintptr_t)data % 16 == 0) && (!TRUTH || (uintptr_t)gt % 16 == 0), "%s: %s must be 16-byte aligned", who, crop ? "data / gt" : "data");
    if (int rc = geom_views(k.g, who, views)) return rc;
    if (int rc = geom_starts(k.g, who, starts)) return rc;
    k.video = video; k.truth = truth; k.data = (float4*)data; k.gt = gt;
    int gx = cdiv((int64_t)S * S, 1024);                             // ~4 pixels per thread
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(clips_from_u8_kernel<TRUTH>, dim3((unsigned)gx, (unsigned)(n * 8), (unsigned)V), dim3(256), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

extern "C" int pc_eval_clips_from_u8(const uint8_t* video, const uint8_t* truth, int F, int H, int W, int h0, int w0, int S,
                                     const int32_t* starts, int n, int f_skip, float* data, float* gt, pc_stream s) {
    const int32_t view[3] = {h0, w0, 0};
    return clips_from_u8<true>("pc_eval_clips_from_u8", video, truth, F, H, W, S, view, view, 1, n, starts, n, f_skip, data, gt, s);
}

extern "C" int pc_clips_from_u8(const uint8_t* video, int F, int H, int W, int h0, int w0, int S, const int32_t* starts, int n, int f_skip,
                                float* data, pc_stream s) {
    const int32_t view[3] = {h0, w0, 0};
    return clips_from_u8<false>("pc_clips_from_u8", video, nullptr, F, H, W, S, view, view, 1, n, starts, n, f_skip, data, nullptr, s);
}

extern "C" int pc_clips_from_u8_views(const uint8_t* video, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                                      const int32_t* starts, int n, int f_skip, float* data, pc_stream s) {
    return clips_from_u8<false>("pc_clips_from_u8_views", video, nullptr, F, H, W, S, nullptr, views, V, view_stride, starts, n, f_skip, data,
                                nullptr, s);
}

extern "C" int pc_video_vote(const float* pred, int n, int C, int label, int32_t* n_correct, pc_stream s) {
    PC_CHECK_ARG(pred && n_correct, "pc_video_vote: null pointer");
    PC_CHECK_ARG(n >= 1 && C >= 1 && (int64_t)n * C < (1ll << 31), "pc_video_vote: n = %d rows of C = %d scores", n, C);
    PC_CHECK_ARG(label >= 0 && label < C, "pc_video_vote: label %d outside [0, %d)", label, C);
    hipLaunchKernelGGL(video_vote_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, pred, n, C, label, n_correct);
    PC_CHECK_LAUNCH("video_vote");
    return PC_OK;
}
