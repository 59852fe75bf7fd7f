// Overlapping clips in time, merged per frame on the device (detect.DetectEngine.set_clip_hop; the window rule: cliphop.h).
//   pc_clip_hop_starts                 host arithmetic: the clip starts of a video of F frames at a hop
//   pc_clip_planes_bytes               host arithmetic: a video's slot planes and its cover bytes
//   pc_clip_planes                     one launch behind each forward:
//     clip_planes_kernel     detectrec.h: merge_to_plane -- merge_group4's merged logit, 0.0f where no view covers, 16 bytes at a time, each
//                            logit fetched once -- into slot (start / hop) % M of the video's planes [M][F][pstride]; the cover bytes
//                            [pstride], the same for every clip of the video, are written by the blocks of the launch's first frame when
//                            the caller asks for them
//   pc_detect_frames_planes_ws_bytes   host arithmetic: the partials of one frame range
//   pc_detect_frames_planes            two launches per frame range, behind a video's last clip:
//     planes_resample_kernel detectrec.h: detect_native_frame, where the value of a plane tap is the mean over the windows that hold the
//                            frame, in ascending window order, by merge_group4's rule (the first value as it is, the others added with
//                            __fadd_rn, one __fdiv_rn by the count when more than one window holds it).  A slot no window filled is never read.
//     planes_records_kernel  detectrec.h: record_from_partials, with the frame taken from the range instead of a clip table and word 6 the
//                            score row of the first clip that holds the frame
// Two clips of one launch never address the same (slot, frame): no atomics, no read-modify-write, nothing to zero, and the order in which a
// video's launches arrive does not matter.
#include "detectrec.h"
#include "cliphop.h"

namespace {

constexpr int PLANES_MAX_FRAMES = PC_PLANES_MAX_FRAMES;

struct PlanesK {
    ClipGeom g;                  // the geometry of the frame the views are crops of (H = Hs, W = Ws)
    const float* logits;
    float* plane;                // [M][F][pstride] merged logits
    uint8_t* cover;              // [pstride] views that cover the pixel, or null: not written by this launch
    size_t pstride;              // Hs * Ws rounded up to a multiple of 4
    int hop, M, bpf_s;
};

struct FramesK {
    const float* plane; const uint8_t* cover; const int32_t* tab;
    uint8_t* mask; uint16_t* prob; int32_t* rec; Partial* part;
    size_t pstride;
    int F, H, W, Hs, Ws, V, f_skip, hop, M, f0, nf, row0, bpf;
};

// grid (bpf_s, n * 8): the frame of slot blockIdx.y into the plane of its window, the cover bytes with the launch's first frame (the entry
// refuses a cover when that frame does not exist)
__global__ __launch_bounds__(256) void clip_planes_kernel(const PlanesK p) {
    const int64_t f = slot_frame(p.g, blockIdx.y);
    if (f < 0) return;
    const int slot = (p.g.starts[blockIdx.y >> 3] / p.hop) % p.M;
    merge_to_plane(p.g, p.logits, blockIdx.y, p.bpf_s, p.plane + ((size_t)slot * p.g.F + (size_t)f) * p.pstride, blockIdx.y == 0 ? p.cover : nullptr);
}

// A tap of one working pixel: the mean over the cnt windows that hold the frame, slot planes s0, s0 + 1, ... (mod M) in ascending window
// order, by merge_group4's rule.
struct MeanTap {
    const float* pf;             // the frame in slot 0
    size_t sstride;              // from one slot to the next
    int s0, cnt, M;
    __device__ __forceinline__ float at(size_t idx) const {
        float acc = pf[(size_t)s0 * sstride + idx];
        int s = s0;
        for (int i = 1; i < cnt; ++i) {
            s = s + 1 == M ? 0 : s + 1;
            acc = __fadd_rn(acc, pf[(size_t)s * sstride + idx]);
        }
        return cnt > 1 ? __fdiv_rn(acc, (float)cnt) : acc;
    }
};

// grid (bpf, nf), bpf = det_views_bpf(H * W): the native frame f0 + blockIdx.y from the windows that hold it
__global__ __launch_bounds__(256) void planes_resample_kernel(const FramesK p) {
    const int64_t f = (int64_t)p.f0 + blockIdx.y;
    const int64_t lo = hop_lo(f, p.f_skip, p.hop), hi = hop_hi(p.F, f, p.f_skip, p.hop);
    const MeanTap tap{p.plane + (size_t)f * p.pstride, (size_t)p.F * p.pstride, (int)(lo % p.M), (int)(hi - lo + 1), p.M};
    detect_native_frame(tap, p.cover, p.tab, f, p.H, p.W, p.Hs, p.Ws, p.mask, p.prob, p.bpf, p.part + (size_t)blockIdx.y * p.bpf + blockIdx.x);
}

// one thread per frame of the range; word 6: the score row of the first clip that holds the frame
__global__ __launch_bounds__(256) void planes_records_kernel(const FramesK p) {
    const int t = blockIdx.x * BT + threadIdx.x;
    if (t >= p.nf) return;
    const int64_t f = (int64_t)p.f0 + t;
    record_from_partials(p.part + (size_t)t * p.bpf, p.bpf, 0, 0, p.row0 + p.V * (int)(hop_lo(f, p.f_skip, p.hop) * p.f_skip + f % p.f_skip),
                         p.rec + (size_t)f * REC_WORDS);
}

}  // namespace

extern "C" int64_t pc_clip_hop_starts(int F, int f_skip, int hop, int32_t* starts, int64_t cap) {
    if (F < 1 || !hop_ok(f_skip, hop)) {
        pc_set_error("pc_clip_hop_starts: F = %d, f_skip = %d, hop = %d (F >= 1, hop a multiple of f_skip in [f_skip, 8 * f_skip])", F, f_skip, hop);
        return PC_E_ARG;
    }
    const int64_t need = hop_clips(F, f_skip, hop);
    if (starts && cap >= need) {
        int64_t at = 0;
        for (int64_t m = 0; m < hop_windows(F, f_skip, hop); ++m)
            for (int j = 0; j < f_skip && m * hop + j < F; ++j) starts[at++] = (int32_t)(m * hop + j);
    }
    return need;
}

extern "C" int64_t pc_clip_planes_bytes(int F, int Hs, int Ws, int f_skip, int hop) {
    if (F < 1 || Hs < 1 || Ws < 1 || (int64_t)Hs * Ws >= (1ll << 31) || !hop_ok(f_skip, hop)) return -1;
    const int64_t ps = (int64_t)plane_stride(Hs, Ws);
    const int64_t frames = (int64_t)hop_slots(f_skip, hop) * F;
    if (frames > (INT64_MAX - ps) / (4 * ps)) return -1;             // beyond 64 bits
    return frames * ps * 4 + ps;                                     // the planes, then the cover bytes (at a multiple of 16)
}

extern "C" int pc_clip_planes(const float* logits, int F, int Hs, int Ws, int S, const int32_t* views, int V, int view_stride, const int32_t* starts,
                              int n, int f_skip, int hop, float* plane, uint8_t* cover, pc_stream s_) {
    const char* who = "pc_clip_planes";
    PlanesK k;
    PC_CHECK_ARG(logits && views && starts && plane, "%s: null pointer", who);
    if (int rc = geom_shape(k.g, who, F, Hs, Ws, S, nullptr)) return rc;
    PC_CHECK_ARG((int64_t)Hs * Ws < (1ll << 31), "%s: frames of %d x %d pixels are outside the 2^31 a frame may hold", who, Hs, Ws);
    PC_CHECK_ARG(S % 4 == 0, "%s: S = %d must be a multiple of 4", who, S);
    if (int rc = geom_counts(k.g, who, V, n, view_stride, f_skip)) return rc;
    PC_CHECK_ARG(hop_ok(f_skip, hop), "%s: hop = %d is no multiple of f_skip = %d in [f_skip, 8 * f_skip]", who, hop, f_skip);
    PC_CHECK_ARG((uintptr_t)logits % 16 == 0 && (uintptr_t)plane % 16 == 0, "%s: logits and plane must be 16-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)cover % 4 == 0, "%s: cover must be 4-byte aligned", who);
    if (int rc = geom_views(k.g, who, views)) return rc;
    if (int rc = geom_starts(k.g, who, starts)) return rc;
    for (int c = 0; c < n; ++c)                                      // a start at or past F holds no frame and is taken, as everywhere
        PC_CHECK_ARG(starts[c] % hop < f_skip && (starts[c] >= F || starts[c] / hop < hop_windows(F, f_skip, hop)),
                     "%s: start %d of clip %d is no clip start of %d frames at hop = %d, f_skip = %d", who, starts[c], c, F, hop, f_skip);
    PC_CHECK_ARG(!cover || starts[0] < F, "%s: cover asked for, but the first clip (start %d) holds no frame below F = %d", who, starts[0], F);
    k.logits = logits; k.plane = plane; k.cover = cover;
    k.pstride = plane_stride(Hs, Ws);
    k.hop = hop; k.M = hop_slots(f_skip, hop);
    k.bpf_s = det_views_bpf((int64_t)Hs * Ws);
    hipLaunchKernelGGL(clip_planes_kernel, dim3((unsigned)k.bpf_s, (unsigned)(n * 8)), dim3(BT), 0, (hipStream_t)s_, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}

extern "C" int64_t pc_detect_frames_planes_ws_bytes(int nf, int H, int W) {
    if (nf < 1 || nf > PLANES_MAX_FRAMES || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 31)) return -1;
    return (int64_t)nf * det_views_bpf((int64_t)H * W) * (int64_t)sizeof(Partial);
}

extern "C" int pc_detect_frames_planes(const float* plane, const uint8_t* cover, int F, int H, int W, int Hs, int Ws, int V, int f_skip, int hop, int f0,
                                       int nf, int row0, const int32_t* dev_tab, uint8_t* mask, uint16_t* prob, int32_t* rec, void* ws, pc_stream s_) {
    const char* who = "pc_detect_frames_planes";
    PC_CHECK_ARG(plane && cover && dev_tab && rec && ws, "%s: null pointer", who);
    PC_CHECK_ARG(F >= 1, "%s: F = %d frames", who, F);
    PC_CHECK_ARG(Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "%s: working frames of %d x %d, native frames of %d x %d", who, Hs, Ws, H, W);
    PC_CHECK_ARG((int64_t)Hs * Ws < (1ll << 31) && (int64_t)H * W < (1ll << 31), "%s: frames of %d x %d or %d x %d pixels are outside the 2^31 a frame may hold",
                 who, Hs, Ws, H, W);
    PC_CHECK_ARG(2 * (int64_t)(H > W ? H : W) < (1ll << 24), "%s: native frames of %d x %d: 2 * max(H, W) must stay below 2^24 (the table's weights)", who, H, W);
    PC_CHECK_ARG(V >= 1 && V <= MAX_VIEWS, "%s: V = %d views outside 1..%d", who, V, MAX_VIEWS);
    PC_CHECK_ARG(hop_ok(f_skip, hop), "%s: hop = %d is no multiple of f_skip = %d in [f_skip, 8 * f_skip]", who, hop, f_skip);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && nf <= PLANES_MAX_FRAMES && (int64_t)f0 + nf <= F, "%s: frames %d .. %d + %d outside the video's %d (a range holds 1..%d)",
                 who, f0, f0, nf, F, PLANES_MAX_FRAMES);
    PC_CHECK_ARG(row0 >= 0 && (int64_t)row0 + (int64_t)V * hop_clips(F, f_skip, hop) <= 0x7fffffff, "%s: row0 = %d", who, row0);
    PC_CHECK_ARG((uintptr_t)plane % 16 == 0 && (uintptr_t)cover % 4 == 0 && (uintptr_t)dev_tab % 4 == 0, "%s: plane must be 16-byte, cover and dev_tab 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)ws % 8 == 0 && (uintptr_t)rec % 4 == 0, "%s: ws must be 8-byte and rec 4-byte aligned", who);
    PC_CHECK_ARG((uintptr_t)prob % 2 == 0, "%s: prob must be 2-byte aligned", who);
    FramesK k;
    k.plane = plane; k.cover = cover; k.tab = dev_tab; k.mask = mask; k.prob = prob; k.rec = rec; k.part = (Partial*)ws;
    k.pstride = plane_stride(Hs, Ws);
    k.F = F; k.H = H; k.W = W; k.Hs = Hs; k.Ws = Ws; k.V = V; k.f_skip = f_skip; k.hop = hop; k.M = hop_slots(f_skip, hop);
    k.f0 = f0; k.nf = nf; k.row0 = row0; k.bpf = det_views_bpf((int64_t)H * W);
    hipStream_t s = (hipStream_t)s_;
    hipLaunchKernelGGL(planes_resample_kernel, dim3((unsigned)k.bpf, (unsigned)nf), dim3(BT), 0, s, k);
    hipLaunchKernelGGL(planes_records_kernel, dim3((unsigned)cdiv(nf, BT)), dim3(BT), 0, s, k);
    PC_CHECK_LAUNCH(who);
    return PC_OK;
}
