// What the mask and the probability map of a multi-view detection share, so that they can never disagree about what was merged:
//   group_pixel      where pixel e of a group of four consecutive pixels lies (the row wrap)
//   merge_group4     the merged logits of four consecutive full-frame pixels (pc_detect_frames_views' rule: the views that cover a pixel in table
//                    order, the first value as it is, the others added with __fadd_rn, one __fdiv_rn by the count when more than one covers)
// merge_group4 is called by detect_frames_views_kernel (mask, box, score) and frame_probs_kernel (the uint16 probability) of detect.hip, and
// by merge_to_plane of detectrec.h (the merged plane of a working frame or of a window, detected at native size behind it).
#pragma once
#include "common.h"
#include "clipgeom.h"

// Pixel e of the group of four that starts at (gy, gx) of a frame W >= 1 wide: at most three rows on.
__device__ __forceinline__ void group_pixel(int gy, int gx, int e, int W, int& y, int& x) {
    y = gy; x = gx + e;
    if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; if (x >= W) { x -= W; ++y; } } }
}

// The group of four consecutive pixels (frame order; it may run over a row's end, and over the frame's end: only the first `ny` exist) that
// starts at pixel px < HW of an H x W frame.  lp: the logits of view 0 for this clip and frame, vstep: floats from one view to the next.
// Where the group lies in one row and a view covers all of it from a 16-byte boundary of its logit row, the view's four values come as one
// float4 (backwards for a mirrored view); otherwise one by one.  -> ny; (gy, gx): the first pixel; num[e]: the views that cover pixel e (0: no
// merged logit, m[e] is then 0.0f); m[e]: the merged logit.  No zero start, so -0.0 and NaN pass through.
__device__ __forceinline__ int merge_group4(const ClipGeom& g, const float* lp, size_t vstep, uint32_t px, uint32_t HW, int& gy, int& gx,
                                            float m[4], int num[4]) {
    const int S = g.S, W = g.W;
    const int ny = (int)(HW - px < 4u ? HW - px : 4u);               // pixels of the group inside the frame
    gy = (int)(px / (uint32_t)W); gx = (int)(px - (uint32_t)gy * (uint32_t)W);
    const bool row = ny == 4 && gx + 3 < W;                          // the group lies in one row
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) num[e] = 0;
    for (int v = 0; v < g.V; ++v) {
        const int h0 = g.vh0[v], w0 = g.vw0[v];
        const bool flip = (g.flips >> v) & 1u;
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
            int y, x;
            group_pixel(gy, gx, e, W, y, x);
            const int ey = y - h0, ex = x - w0;
            if (e < ny && ey >= 0 && ey < S && ex >= 0 && ex < S) {
                const float t = lv[(size_t)ey * S + (flip ? S - 1 - ex : ex)];
                acc[e] = num[e] ? __fadd_rn(acc[e], t) : t;
                ++num[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = num[e] > 1 ? __fdiv_rn(acc[e], (float)num[e]) : acc[e];
    return ny;
}

