// Detection on a resized working frame, results at native size (detect.DetectEngine.set_working_frame): the views are crops of an
// Hs x Ws working frame, the masks, boxes, scores and probabilities stand on the H x W frame the video came in.
//   pc_resample_tables                  host arithmetic: per native row and column the first tap and the weight of the second, half-pixel
//                                       centres (cv2.INTER_LINEAR / align_corners=False), the index exact in 64-bit integers
//   pc_detect_frames_scaled_ws_bytes    host arithmetic: the partials, then the merged plane (a float and a cover byte per working pixel)
//   pc_detect_frames_scaled             two traversals and the records kernel:
//     merge_plane_kernel     the working frame in groups of four (viewmerge.h: merge_group4, the rule of pc_detect_frames_views bit for
//                            bit): merged logit and cover count of every working pixel into the plane in `ws`, each logit fetched once
//     resample_kernel        the native frame in groups of four: up to four taps of the plane per pixel, every product and sum one fp32
//                            round-to-nearest operation, a tap of zero weight not read; then seg_positive, mask, box, score and (if asked
//                            for) the uint16 probability of pc_frame_probs -- one pass, no second walk over the logits
//     detect_records_kernel  detectrec.h: the partials in block order -> the 8-word record
// The plane of one (clip, frame) slot is padded to a multiple of four pixels, so that a group's four floats and four cover bytes always go
// out as one 16-byte and one 4-byte store.  No atomics of any kind; nothing has to be zeroed in front of the launch.
#include <cstring>

#include "common.h"
#include "evalpred.h"
#include "clipgeom.h"
#include "viewmerge.h"
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

inline size_t plane_stride(int Hs, int Ws) { return ((size_t)Hs * Ws + 3) & ~(size_t)3; }

inline bool scaled_shape_ok(int n, int Hs, int Ws, int H, int W) {
    return n >= 1 && n <= MAX_CLIPS && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1 && (int64_t)Hs * Ws < (1ll << 31) && (int64_t)H * W < (1ll << 31) &&
           2 * (int64_t)(H > W ? H : W) < (1ll << 24);
}

// grid (bpf_s, n * 8): the groups of four of detect_frames_views_kernel over the working frame.  The padding of a slot's last group takes
// merge_group4's values for pixels that do not exist (0.0f, cover 0); nothing reads it.
__global__ __launch_bounds__(256) void merge_plane_kernel(const ScaleK p) {
    const ClipGeom& g = p.d.g;
    const int c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)g.starts[c] + (int64_t)k * g.f_skip;
    if (f >= g.F) return;                                            // a frame past the end: nothing read, nothing written
    const uint32_t HW = (uint32_t)g.H * (uint32_t)g.W, total4 = (HW + 3u) >> 2;
    const size_t per = (size_t)g.S * g.S;
    const float* lp = p.d.logits + ((size_t)c * 8 + k) * per;        // view v: + v * view_stride * 8 * per
    const size_t vstep = (size_t)g.view_stride * 8 * per;
    float* pl = p.plane + (size_t)blockIdx.y * p.pstride;
    uint8_t* cv = p.cover + (size_t)blockIdx.y * p.pstride;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)p.bpf_s * BT) {
        const uint32_t px = idx << 2;
        float mg[4];
        int num[4], gy, gx;
        merge_group4(g, lp, vstep, px, HW, gy, gx, mg, num);
        f32x4 q;
        q[0] = mg[0]; q[1] = mg[1]; q[2] = mg[2]; q[3] = mg[3];
        *(f32x4*)(pl + px) = q;
        *(uint32_t*)(cv + px) = (uint32_t)num[0] | ((uint32_t)num[1] << 8) | ((uint32_t)num[2] << 16) | ((uint32_t)num[3] << 24);
    }
}

// One tap row of the bilinear rule: the value at column pair (ix, ix + 1) of plane row r with the second weight wx1; `ok` is cleared when a
// tap that is read has no cover.  A tap of zero weight is not read.
__device__ __forceinline__ float tap_row(const float* pl, const uint8_t* cv, size_t r, int ix, int ix1, float wx0, float wx1, bool& ok) {
    const float a = pl[r + ix];
    ok = ok && cv[r + ix] != 0;
    if (wx1 == 0.0f) return a;
    const float b = pl[r + ix1];
    ok = ok && cv[r + ix1] != 0;
    return __fadd_rn(__fmul_rn(a, wx0), __fmul_rn(b, wx1));
}

// grid (bpf, n * 8), bpf = det_views_bpf(H * W): the native frame in groups of four consecutive pixels (frame order, a group may run over a
// row's end).  The grouping depends on H, W alone, so the order of the sums is the same with any mask or prob or none.  The table's indices
// are clamped into the plane: a table that is not pc_resample_tables' for these sizes gives wrong values, never an access outside `ws`.
__global__ __launch_bounds__(256) void resample_kernel(const ScaleK p) {
    const ClipGeom& g = p.d.g;
    const int c = blockIdx.y >> 3, k = blockIdx.y & 7;
    const int64_t f = (int64_t)g.starts[c] + (int64_t)k * g.f_skip;
    if (f >= g.F) return;                                            // a frame past the end: nothing read, nothing written
    const int W = p.W, Hs = g.H, Ws = g.W;
    const uint32_t HW = (uint32_t)p.H * (uint32_t)W, total4 = (HW + 3u) >> 2;
    const float* pl = p.plane + (size_t)blockIdx.y * p.pstride;
    const uint8_t* cv = p.cover + (size_t)blockIdx.y * p.pstride;
    const int32_t* rowt = p.tab;
    const int32_t* colt = p.tab + 2 * (size_t)p.H;
    uint8_t* mf = p.d.mask ? p.d.mask + (size_t)f * HW : nullptr;
    uint16_t* pf = p.prob ? p.prob + (size_t)f * HW : nullptr;
    double sum = 0.0;
    int cnt = 0, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    for (uint32_t idx = blockIdx.x * BT + threadIdx.x; idx < total4; idx += (uint32_t)p.d.bpf * BT) {
        const uint32_t px = idx << 2;
        const int ny = (int)(HW - px < 4u ? HW - px : 4u);
        const int gy = (int)(px / (uint32_t)W), gx = (int)(px - (uint32_t)gy * (uint32_t)W);
        uint32_t bits = 0, q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= ny) continue;
            int y = gy, x = gx + e;
            if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; } } }     // W >= 1: at most three rows on
            const int iy = min(max(rowt[2 * y], 0), Hs - 1), iy1 = min(iy + 1, Hs - 1);
            const int ix = min(max(colt[2 * x], 0), Ws - 1), ix1 = min(ix + 1, Ws - 1);
            const float wy1 = __int_as_float(rowt[2 * y + 1]), wx1 = __int_as_float(colt[2 * x + 1]);
            const float wy0 = __fsub_rn(1.0f, wy1), wx0 = __fsub_rn(1.0f, wx1);
            bool ok = true;
            float v = tap_row(pl, cv, (size_t)iy * Ws, ix, ix1, wx0, wx1, ok);
            if (wy1 != 0.0f) {
                const float bot = tap_row(pl, cv, (size_t)iy1 * Ws, ix, ix1, wx0, wx1, ok);
                v = __fadd_rn(__fmul_rn(v, wy0), __fmul_rn(bot, wy1));
            }
            if (!ok) continue;                                       // a tap that was read has no cover: background, probability 0
            const float sg = 1.0f / (1.0f + expf(-v));
            if (v == v) q[e] = __float2uint_rn(sg * (float)PC_PROB_ONE);
            if (seg_positive(v)) {
                bits |= 1u << (8 * e);
                sum += (double)sg;
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
        if (pf) {
            uint16_t* o = pf + px;
            if (ny == 4 && ((uintptr_t)o & 7) == 0) {
                *(uint2*)o = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
            } else {
                for (int e = 0; e < ny; ++e) o[e] = (uint16_t)q[e];
            }
        }
    }
    block_partial(sum, cnt, x0, y0, x1, y1, p.d.part + (size_t)blockIdx.y * p.d.bpf + blockIdx.x);
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
