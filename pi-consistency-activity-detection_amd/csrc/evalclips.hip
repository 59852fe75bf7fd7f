// Evaluation input on the device: what the reference's eval loop does per video on the host before the network sees a clip
// (evaluate_ucf101.py:79-101 on the centre-cropped frames and truth of datasets/ucf_dataloader_eval.py:100-106) and the class vote
// behind it (:139-146), from the decoded uint8 frames and uint8 truth already in HBM.
//   pc_truth_frame_flags   per frame, the number of non-zero truth pixels inside the crop: decides which clips are kept (:95-96)
//   pc_eval_clips_from_u8  up to 32 clips of one video straight into the NDHWC tensor the stem reads and the frame-major truth
//                          pc_seg_frame_counts takes; HBM-bound, 4 bytes read and 20 written per pixel
//   pc_clips_from_u8       the same kernel without the truth side (unlabelled video: picons_amd/detect.py)
//   pc_clips_from_u8_views pc_clips_from_u8 for V views (crops at their own offsets, some mirrored left-right) of the clips in one launch
//   pc_video_vote          argmax(mean(predictions, axis=0)) == label, rows added in order in fp32 as numpy adds them
#include "common.h"
#include "evalpred.h"

namespace {

constexpr int MAX_CLIPS = 32;

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

struct EvalClipsK {
    const uint8_t* video; const uint8_t* truth;
    int F, H, W, h0, w0, S, f_skip;
    int starts[MAX_CLIPS];
    float4* data; float* gt;
};

// blockIdx.y = clip * 8 + frame of the clip, blockIdx.x strides over the frame's S*S pixels: one thread per pixel writes one whole float4
// (a wave: 1 KiB contiguous) and one truth float (256 B contiguous).  The source bytes of a cropped RGB row start at any byte address, so
// they are read as bytes; consecutive lanes read consecutive 3-byte pixels of one row.
// TRUTH = false (pc_clips_from_u8): the same body without the truth side; p.truth and p.gt are never touched.
template <bool TRUTH>
__global__ __launch_bounds__(256) void eval_clips_from_u8_kernel(const EvalClipsK p) {
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);        // img / 255. in float64, then the float32 cast: once per block
    __syncthreads();
    const int c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    const int total = p.S * p.S;
    float4* data = p.data + (size_t)blockIdx.y * total;
    float* gt = TRUTH ? p.gt + (size_t)blockIdx.y * total : nullptr;
    if (f >= p.F) {                                                  // a frame past the end: zeros, nothing read (evaluate_ucf101.py:89-91)
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
            data[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (TRUTH) gt[idx] = 0.f;
        }
        return;
    }
    const uint8_t* vf = p.video + (((size_t)f * p.H + p.h0) * p.W + p.w0) * 3;
    const uint8_t* tf = TRUTH ? p.truth + ((size_t)f * p.H + p.h0) * p.W + p.w0 : nullptr;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / p.S, x = idx - y * p.S;
        const uint8_t* px = vf + ((size_t)y * p.W + x) * 3;
        data[idx] = make_float4(lut[px[0]], lut[px[1]], lut[px[2]], 0.f);
        if (TRUTH) gt[idx] = (float)tf[(size_t)y * p.W + x];         // the value itself: the reference counts pred + gt == 2
    }
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

// The checks and the launch pc_eval_clips_from_u8 (TRUTH) and pc_clips_from_u8 share; `who` names the entry in the messages.
template <bool TRUTH>
static int clips_from_u8(const char* who, const uint8_t* video, const uint8_t* truth, int F, int H, int W, int h0, int w0, int S,
                         const int32_t* starts, int n, int f_skip, float* data, float* gt, pc_stream s) {
    PC_CHECK_ARG(video && starts && data && (!TRUTH || (truth && gt)), "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768 && h0 >= 0 && w0 >= 0 && (int64_t)h0 + S <= H && (int64_t)w0 + S <= W,
                 "%s: %d frames, crop %d+%d x %d+%d outside %d x %d", who, F, h0, S, w0, S, H, W);
    PC_CHECK_ARG(n >= 1 && n <= MAX_CLIPS, "%s: n = %d clips outside 1..%d", who, n, MAX_CLIPS);
    PC_CHECK_ARG(f_skip >= 1, "%s: f_skip = %d", who, f_skip);
    PC_CHECK_ARG(((uintptr_t)data % 16 == 0) && (!TRUTH || (uintptr_t)gt % 16 == 0), "%s: data / gt must be 16-byte aligned", who);
    EvalClipsK k;
    k.video = video; k.truth = truth; k.F = F; k.H = H; k.W = W; k.h0 = h0; k.w0 = w0; k.S = S; k.f_skip = f_skip;
    k.data = (float4*)data; k.gt = gt;
    for (int c = 0; c < MAX_CLIPS; ++c) {
        if (c < n) PC_CHECK_ARG(starts[c] >= 0, "%s: start %d of clip %d is negative", who, starts[c], c);
        k.starts[c] = c < n ? starts[c] : 0;
    }
    int gx = cdiv((int64_t)S * S, 1024);                             // ~4 pixels per thread
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(eval_clips_from_u8_kernel<TRUTH>, dim3((unsigned)gx, (unsigned)(n * 8)), dim3(256), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

extern "C" int pc_eval_clips_from_u8(const uint8_t* video, const uint8_t* truth, int F, int H, int W, int h0, int w0, int S,
                                     const int32_t* starts, int n, int f_skip, float* data, float* gt, pc_stream s) {
    return clips_from_u8<true>("pc_eval_clips_from_u8", video, truth, F, H, W, h0, w0, S, starts, n, f_skip, data, gt, s);
}

extern "C" int pc_clips_from_u8(const uint8_t* video, int F, int H, int W, int h0, int w0, int S, const int32_t* starts, int n, int f_skip,
                                float* data, pc_stream s) {
    return clips_from_u8<false>("pc_clips_from_u8", video, nullptr, F, H, W, h0, w0, S, starts, n, f_skip, data, nullptr, s);
}

extern "C" int pc_video_vote(const float* pred, int n, int C, int label, int32_t* n_correct, pc_stream s) {
    PC_CHECK_ARG(pred && n_correct, "pc_video_vote: null pointer");
    PC_CHECK_ARG(n >= 1 && C >= 1 && (int64_t)n * C < (1ll << 31), "pc_video_vote: n = %d rows of C = %d scores", n, C);
    PC_CHECK_ARG(label >= 0 && label < C, "pc_video_vote: label %d outside [0, %d)", label, C);
    hipLaunchKernelGGL(video_vote_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, pred, n, C, label, n_correct);
    PC_CHECK_LAUNCH("video_vote");
    return PC_OK;
}

// ---------------------------------------------------------------------- views (detect.DetectEngine, tile / flip)
namespace {

constexpr int MAX_VIEWS = 32;

struct ClipViewsK {
    const uint8_t* video;
    int F, H, W, S, f_skip, n, view_stride;
    int starts[MAX_CLIPS];
    int vh0[MAX_VIEWS], vw0[MAX_VIEWS];
    uint32_t flips;                                                  // bit v: view v is mirrored left-right
    float4* data;
};

// pc_clips_from_u8 for V views (crops at their own offsets, some mirrored) of the n clips in one launch: blockIdx.y = (view * n + clip) * 8 +
// frame of the clip, written at clip slot view * view_stride + clip; blockIdx.x strides over the S*S pixels, one whole float4 per thread as
// in eval_clips_from_u8_kernel.  A mirrored view reads its row backwards: consecutive lanes, descending 3-byte pixels of one row.
__global__ __launch_bounds__(256) void clips_from_u8_views_kernel(const ClipViewsK p) {
    __shared__ float lut[256];
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);        // the table of eval_clips_from_u8_kernel
    __syncthreads();
    const int v = blockIdx.y / (p.n * 8), ck = blockIdx.y - v * (p.n * 8);
    const int c = ck >> 3, k = ck & 7;
    const int64_t f = (int64_t)p.starts[c] + (int64_t)k * p.f_skip;
    const int S = p.S, total = S * S;
    float4* data = p.data + (((size_t)v * p.view_stride + c) * 8 + k) * total;
    if (f >= p.F) {                                                  // a frame past the end: zeros, nothing read
        for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) data[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const bool flip = (p.flips >> v) & 1u;
    const uint8_t* vf = p.video + (((size_t)f * p.H + p.vh0[v]) * p.W + p.vw0[v]) * 3;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
        const int y = idx / S, x = idx - y * S;
        const uint8_t* px = vf + ((size_t)y * p.W + (flip ? S - 1 - x : x)) * 3;
        data[idx] = make_float4(lut[px[0]], lut[px[1]], lut[px[2]], 0.f);
    }
}

}  // namespace

extern "C" int pc_clips_from_u8_views(const uint8_t* video, int F, int H, int W, int S, const int32_t* views, int V, int view_stride,
                                      const int32_t* starts, int n, int f_skip, float* data, pc_stream s) {
    const char* who = "pc_clips_from_u8_views";
    PC_CHECK_ARG(video && views && starts && data, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768 && S <= H && S <= W, "%s: %d frames, crop of %d outside %d x %d", who, F, S, H, W);
    PC_CHECK_ARG(V >= 1 && V <= MAX_VIEWS, "%s: V = %d views outside 1..%d", who, V, MAX_VIEWS);
    PC_CHECK_ARG(n >= 1 && n <= MAX_CLIPS, "%s: n = %d clips outside 1..%d", who, n, MAX_CLIPS);
    PC_CHECK_ARG(view_stride >= n, "%s: view_stride = %d is below the n = %d clips of a view", who, view_stride, n);
    PC_CHECK_ARG(f_skip >= 1, "%s: f_skip = %d", who, f_skip);
    PC_CHECK_ARG((uintptr_t)data % 16 == 0, "%s: data must be 16-byte aligned", who);
    ClipViewsK k;
    k.video = video; k.F = F; k.H = H; k.W = W; k.S = S; k.f_skip = f_skip; k.n = n; k.view_stride = view_stride; k.flips = 0;
    k.data = (float4*)data;
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
    int gx = cdiv((int64_t)S * S, 1024);                             // ~4 pixels per thread
    if (gx > 1024) gx = 1024;
    hipLaunchKernelGGL(clips_from_u8_views_kernel, dim3((unsigned)gx, (unsigned)(V * n * 8)), dim3(256), 0, (hipStream_t)s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
