// Truth given as boxes, painted on the device (evalstep.BoxTruth; EvalEngine.add_video, detect.DetectEngine.score / sweep): a whole video's
// truth map uint8 [F][H][W] from a table of rects int32 [F][R][5] = (x0, x1, y0, y1, value), half-open, frame coordinates.
//   pc_paint_boxes   paint_boxes_kernel on a grid of bpf blocks per frame (det_views_bpf: a function of H * W alone, at most 64).  Wave 0 of a
//                    block reads the frame's R rects once, intersects each with the frame, drops those that paint nothing (empty, or a zero
//                    low byte of the value) and leaves the rest in LDS in table order (a ballot and a prefix count: the order is kept).  Then
//                    each thread strides over its share of the frame's four-pixel groups: a pixel's byte is the value of the LAST rect of the
//                    table that contains it, 0 if none does (binary: 1 for every value) -- what painting the rects in order gives --, and the
//                    group's bytes go out as one dword where the address allows (a frame of odd H * W starts at any byte), bytes otherwise.
// SAFE BY CONSTRUCTION: a rect word never becomes part of an address.  A thread owns output bytes -- groups below the frame's end, of a frame
// inside the range the host checked -- and only TESTS whether a rect contains them.  A rect that reaches outside the frame, or holds any
// 32-bit pattern whatever, is clamped into [0, W] x [0, H] before its width is formed (so nothing overflows) and is thereby intersected with
// the frame: the table can make the map wrong, never make the kernel write outside it.
// Write-only: nothing is read from `truth`, no fill precedes the launch, every byte of an addressed frame is written exactly once and no other
// byte at all.  No atomics, no floating point, nothing waits on another block, every loop's trip count is known before it starts: bit-identical
// from run to run.  The floor is nf * H * W bytes of stores.
#include "detectrec.h"

namespace {

constexpr int MAX_GRID = 1 << 23;                                    // blocks of one launch: 2^31 threads

struct BoxK {
    const int32_t* rects; uint8_t* truth;                            // frame 0 of the launch's frames
    int R, H, W, bpf, binary;
};

// The first ny bytes of a group (byte e of `bytes`: pixel e): one dword where the address allows, bytes otherwise.
__device__ __forceinline__ void store_bytes4(uint8_t* m, uint32_t bytes, int ny) {
    if (ny == 4 && ((uintptr_t)m & 3) == 0) {
        *(uint32_t*)m = bytes;
    } else {
        for (int e = 0; e < ny; ++e) m[e] = (uint8_t)(bytes >> (8 * e));
    }
}

// grid (frames * bpf): block x is share x % bpf of frame x / bpf.  A group past the frame's end is not written.
__global__ __launch_bounds__(256) void paint_boxes_kernel(const BoxK p) {
    __shared__ int4 box[PC_BOX_MAX];                                 // x0, width, y0, height of a rect that paints, inside the frame
    __shared__ uint32_t val[PC_BOX_MAX];
    __shared__ int nbox;
    const int tid = threadIdx.x, W = p.W, H = p.H;
    const uint32_t HW = (uint32_t)H * (uint32_t)W, total4 = (HW + 3u) >> 2;
    const uint32_t fr = blockIdx.x / (uint32_t)p.bpf, part = blockIdx.x % (uint32_t)p.bpf, stride = (uint32_t)p.bpf * BT;

    if (tid < 64) {                                                  // wave 0, all of it: the ballot sees 64 lanes
        int4 b = make_int4(0, 0, 0, 0);
        uint32_t v = 0;
        bool paints = false;
        if (tid < p.R) {
            const int32_t* r = p.rects + ((size_t)fr * (size_t)p.R + (size_t)tid) * PC_BOX_WORDS;
            const int x0 = min(max(r[0], 0), W), x1 = min(max(r[1], 0), W), y0 = min(max(r[2], 0), H), y1 = min(max(r[3], 0), H);
            b = make_int4(x0, x1 - x0, y0, y1 - y0);                 // all four in [0, W] / [0, H]: the differences cannot overflow
            v = (uint32_t)r[4] & 255u;
            paints = b.y > 0 && b.w > 0 && v != 0u;
            if (p.binary) v = 1u;
        }
        const uint64_t m = __ballot(paints);
        if (paints) {
            const int at = __popcll(m & ((1ull << tid) - 1ull));     // the painting rects in front of this one: table order is kept
            box[at] = b;
            val[at] = v;
        }
        if (tid == 0) nbox = __popcll(m);
    }
    __syncthreads();
    const int n = nbox;
    uint8_t* tf = p.truth + (size_t)fr * HW;

    for (uint32_t gr = part * BT + tid; gr < total4; gr += stride) {
        const uint32_t px = gr << 2;
        const int ny = (int)(HW - px < 4u ? HW - px : 4u);
        const int gy = (int)(px / (uint32_t)W), gx = (int)(px - (uint32_t)gy * (uint32_t)W);
        int y[4], x[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) group_pixel(gy, gx, e, W, y[e], x[e]);   // a pixel past the frame's end has y >= H: no rect holds it
        uint32_t bytes = 0;
        for (int r = 0; r < n; ++r) {                                // block-uniform: every lane reads the same LDS words
            const int4 b = box[r];
            const uint32_t v = val[r];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = (uint32_t)(x[e] - b.x) < (uint32_t)b.y && (uint32_t)(y[e] - b.z) < (uint32_t)b.w;
                bytes = in ? (bytes & ~(0xffu << (8 * e))) | (v << (8 * e)) : bytes;
            }
        }
        store_bytes4(tf + px, bytes, ny);
    }
}

}  // namespace

extern "C" int pc_paint_boxes(const int32_t* rects, int R, int F, int H, int W, int f0, int nf, int binary, uint8_t* truth, pc_stream s) {
    const char* who = "pc_paint_boxes";
    PC_CHECK_ARG(rects && truth, "%s: null pointer (rects or truth)", who);
    PC_CHECK_ARG(F >= 1 && H >= 1 && W >= 1, "%s: F = %d frames of %d x %d are outside what a map holds", who, F, H, W);
    PC_CHECK_ARG((int64_t)H * W < (1ll << 31), "%s: frames of %d x %d pixels are beyond the 2^31 a frame may hold", who, H, W);
    PC_CHECK_ARG(R >= 1 && R <= PC_BOX_MAX, "%s: R = %d rects per frame outside 1..%d", who, R, PC_BOX_MAX);
    PC_CHECK_ARG(f0 >= 0 && nf >= 1 && (int64_t)f0 + nf <= F, "%s: frames f0 = %d, nf = %d outside the %d of the map", who, f0, nf, F);
    PC_CHECK_ARG((uintptr_t)rects % 4 == 0, "%s: rects must be 4-byte aligned", who);
    const size_t HW = (size_t)H * (size_t)W;
    const int bpf = det_views_bpf((int64_t)HW);
    const int per = MAX_GRID / bpf;                                  // frames of one launch (a video is one launch; only a map of millions of frames is cut)
    BoxK k;
    k.R = R; k.H = H; k.W = W; k.bpf = bpf; k.binary = binary != 0;
    for (int64_t c0 = 0; c0 < nf; c0 += per) {
        const int n = (int)(nf - c0 < per ? nf - c0 : per);
        const size_t fa = (size_t)f0 + (size_t)c0;
        k.rects = rects + fa * (size_t)R * PC_BOX_WORDS;
        k.truth = truth + fa * HW;
        hipLaunchKernelGGL(paint_boxes_kernel, dim3((unsigned)(n * bpf)), dim3(BT), 0, (hipStream_t)s, k);
        PC_CHECK_LAUNCH(who);
    }
    return PC_OK;
}
