// Detection on a resized working frame, results at native size (detect.DetectEngine.set_working_frame): the views are crops of an
// Hs x Ws working frame, the masks, boxes, scores and probabilities stand on the H x W frame the video came in.
//   pc_resample_tables                  host arithmetic: per native row and column the first tap and the weight of the second, half-pixel
//                                       centres (cv2.INTER_LINEAR / align_corners=False), the index exact in 64-bit integers
//   pc_detect_frames_scaled_ws_bytes    host arithmetic: the partials, then the merged plane (a float and a cover byte per working pixel)
//   pc_detect_frames_scaled             two traversals and the records kernel:
//     merge_plane_kernel     detectrec.h: merge_to_plane, the working frame in groups of four (merge_group4, the rule of
//                            pc_detect_frames_views bit for bit): merged logit and cover count of every working pixel into the (clip,
//                            frame) slot's plane in `ws`, each logit fetched once
//     resample_kernel        detectrec.h: detect_native_frame over one plane, the native frame in groups of four: up to four taps of
//                            the plane per pixel, every product and sum one fp32 round-to-nearest operation, a tap of zero weight not read;
//                            then seg_positive, mask, box, score and (if asked for) the uint16 probability of pc_frame_probs -- one pass,
//                            no second walk over the logits
//     detect_records_kernel  detectrec.h: the partials in block order -> the 8-word record
// No atomics of any kind; nothing has to be zeroed in front of the launch.
#include <cstring>

#include "detectrec.h"

namespace {

struct ScaleK {
    DetectK d;                   // logits, mask, rec, part (native bpf), row0; g: the geometry of the WORKING frame (H = Hs, W = Ws)
    float* plane;                // [n * 8][pstride] merged logits
    uint8_t* cover;              // [n * 8][pstride] views that cover the working pixel
    const int32_t* tab;          // pc_resample_tables: rows [H][2], then columns [W][2]
    uint16_t* prob;
    size_t pstride;              // Hs * Ws rounded up to a multiple of 4
    int H, W, bpf_s;             // the native frame; blocks per frame of the merge traversal
};

inline bool scaled_shape_ok(int n, int Hs, int Ws, int H, int W) {
    return n >= 1 && n <= MAX_CLIPS && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && (int64_t)Hs * Ws < (1ll << 31) && (int64_t)H * W < (1ll << 31) &&
           2 * (int64_t)(H > W ? H : W) < (1ll << 24);
}

// grid (bpf_s, n * 8): the working frame of slot blockIdx.y into its plane and cover
__global__ __launch_bounds__(256) void merge_plane_kernel(const ScaleK p) {
    if (slot_frame(p.d.g, blockIdx.y) < 0) return;
    merge_to_plane(p.d.g, p.d.logits, blockIdx.y, p.bpf_s, p.plane + (size_t)blockIdx.y * p.pstride, p.cover + (size_t)blockIdx.y * p.pstride);
}

struct PlaneTap {                // a tap of the slot's one plane
    const float* pl;
    __device__ __forceinline__ float at(size_t idx) const { return pl[idx]; }
};

// grid (bpf, n * 8), bpf = det_views_bpf(H * W): the native frame from the plane of slot blockIdx.y
__global__ __launch_bounds__(256) void resample_kernel(const ScaleK p) {
    const int64_t f = slot_frame(p.d.g, blockIdx.y);
    if (f < 0) return;
    const PlaneTap tap{p.plane + (size_t)blockIdx.y * p.pstride};
    detect_native_frame(tap, p.cover + (size_t)blockIdx.y * p.pstride, p.tab, f, p.H, p.W, p.d.g.H, p.d.g.W, p.d.mask, p.prob, p.d.bpf,
                        p.d.part + (size_t)blockIdx.y * p.d.bpf + blockIdx.x);
}

inline int64_t partial_bytes(int n, int H, int W) { return (int64_t)n * 8 * det_views_bpf((int64_t)H * W) * (int64_t)sizeof(Partial); }

// One axis of the table: destination index d of D from a source of length L -> (i0, bits of float32 w1).
inline void resample_axis(int L, int D, int32_t* out) {
    const int64_t den = 2 * (int64_t)D;
    for (int d = 0; d < D; ++d) {
        const int64_t num = (2 * (int64_t)d + 1) * L - D;
        int64_t i0 = num >= 0 ? num / den : -((-num + den - 1) / den);      // floor
        int64_t r = num - i0 * den;
        if (i0 < 0) { i0 = 0; r = 0; }
        if (i0 >= L - 1) { i0 = L - 1; r = 0; }
        const float w1 = (float)r / (float)den;                             // both exact in float32 (< 2^24): one rounding
        int32_t b;
        memcpy(&b, &w1, 4);
        out[2 * d] = (int32_t)i0;
        out[2 * d + 1] = b;
    }
}

}  // namespace

extern "C" int64_t pc_resample_tables(int Hs, int Ws, int H, int W, int32_t* tab, int64_t cap) {
    if (Hs < 1 || Ws < 1 || H < 1 || W < 1 || 2 * (int64_t)(H > W ? H : W) >= (1ll << 24)) {
        pc_set_error("pc_resample_tables: %d x %d -> %d x %d (sizes >= 1, 2 * max(H, W) < 2^24)", Hs, Ws, H, W);
        return PC_E_ARG;
    }
    const int64_t need = 2 * ((int64_t)H + W);
    if (tab && cap >= need) {
        resample_axis(Hs, H, tab);
        resample_axis(Ws, W, tab + 2 * (size_t)H);
    }
    return need;
}

extern "C" int64_t pc_detect_frames_scaled_ws_bytes(int n, int Hs, int Ws, int H, int W) {
    if (!scaled_shape_ok(n, Hs, Ws, H, W)) return -1;
    // the partials; 16 bytes so that the plane starts at a 16-byte boundary behind an 8-byte aligned ws; a float and a byte per plane pixel
    return partial_bytes(n, H, W) + 16 + (int64_t)n * 8 * (int64_t)plane_stride(Hs, Ws) * 5;
}

extern "C" int pc_detect_frames_scaled(const float* logits, int F, int H, int W, int Hs, int Ws, int S, const int32_t* views, int V, int view_stride,
                                       const int32_t* starts, int n, int f_skip, int row0, const int32_t* dev_tab, uint8_t* mask, uint16_t* prob,
                                       int32_t* rec, void* ws, pc_stream s_) {
    const char* who = "pc_detect_frames_scaled";
    ScaleK k;
    PC_CHECK_ARG(dev_tab != nullptr, "%s: null pointer (dev_tab)", who);
    if (int rc = detect_args(k.d.g, who, logits, F, Hs, Ws, S, nullptr, views, V, view_stride, starts, n, f_skip, row0, rec, ws)) return rc;
    PC_CHECK_ARG(H >= 1 && W >= 1, "%s: native frames of %d x %d", who, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: native frames of %d x %d pixels are outside the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(2 * (int64_t)(H > W ? H : W) < (1ll << 24), "%s: native frames of %d x %d: 2 * max(H, W) must stay below 2^24 (the table's weights)", who, H, W);
    PC_CHECK_ARG((uintptr_t)dev_tab % 4 == 0, "%s: dev_tab must be 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)prob % 2 == 0, "%s: prob must be 2-byte aligned", who);
    k.d.logits = logits; k.d.mask = mask; k.d.rec = rec; k.d.part = (Partial*)ws; k.d.row0 = row0;
    k.d.bpf = det_views_bpf((int64_t)H * W);
    k.bpf_s = det_views_bpf((int64_t)Hs * Ws);
    k.pstride = plane_stride(Hs, Ws);
    const uintptr_t base = ((uintptr_t)ws + (uintptr_t)partial_bytes(n, H, W) + 15) & ~(uintptr_t)15;
    k.plane = (float*)base;
    k.cover = (uint8_t*)(base + (size_t)n * 8 * k.pstride * sizeof(float));
    k.tab = dev_tab; k.prob = prob; k.H = H; k.W = W;
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(merge_plane_kernel, dim3((unsigned)k.bpf_s, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)k.d.bpf, (unsigned)(n * 8)), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(detect_records_kernel, dim3((unsigned)cdiv(n * 8, BT)), dim3(BT), 0, s, k.d, n * 8, 0, 0, V);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
