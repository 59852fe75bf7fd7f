// What the clip kernels of evalclips.hip (video -> clips) and detect.hip (logits of the clips -> video) agree on: which frames a launch's clips
// hold and where in the frame each view of a clip lies.  One block of kernel arguments and the host checks that fill it, so that a change to
// how a start, a crop or a frame past the end is treated reaches every entry.
//   frame k of clip c is video frame starts[c] + k * f_skip; a frame at or past F does not exist
//   view v of clip c is the S x S crop at (vh0[v], vw0[v]) of the H x W frame, mirrored left-right if bit v of flips is set, and lies at
//   clip slot v * view_stride + c of the clip tensor.  A centre-crop entry is the one view (h0, w0, 0) at stride n.
// The geom_* helpers refuse with PC_E_ARG and a message that begins with `who`, the entry's name; an entry calls them in the order shape,
// counts, views, starts, with its own checks in between.
#pragma once
#include "common.h"

constexpr int MAX_CLIPS = 32;                                        // clips of one launch
constexpr int MAX_VIEWS = 32;                                        // views of one launch

struct ClipGeom {
    int F, H, W, S, f_skip, n, V, view_stride;
    int starts[MAX_CLIPS];
    int vh0[MAX_VIEWS], vw0[MAX_VIEWS];
    uint32_t flips;                                                  // bit v: view v is mirrored left-right
};

// crop: the (h0, w0) of a centre-crop entry, or null for an entry whose crops come in a view table (geom_views checks each of them)
inline int geom_shape(ClipGeom& g, const char* who, int F, int H, int W, int S, const int32_t* crop) {
    const bool ok = F >= 1 && H >= 1 && W >= 1 && S >= 1 && S <= 32768;
    if (crop) {
        const int h0 = crop[0], w0 = crop[1];
        PC_CHECK_ARG(ok && h0 >= 0 && w0 >= 0 && (int64_t)h0 + S <= H && (int64_t)w0 + S <= W, "%s: %d frames, crop %d+%d x %d+%d outside %d x %d", who,
                     F, h0, S, w0, S, H, W);
    } else {
        PC_CHECK_ARG(ok && S <= H && S <= W, "%s: %d frames, crop of %d outside %d x %d", who, F, S, H, W);
    }
    g.F = F; g.H = H; g.W = W; g.S = S;
    return PC_OK;
}

inline int geom_counts(ClipGeom& g, const char* who, int V, int n, int view_stride, int f_skip) {
    PC_CHECK_ARG(V >= 1 && V <= MAX_VIEWS, "%s: V = %d views outside 1..%d", who, V, MAX_VIEWS);
    PC_CHECK_ARG(n >= 1 && n <= MAX_CLIPS, "%s: n = %d clips outside 1..%d", who, n, MAX_CLIPS);
    PC_CHECK_ARG(view_stride >= n, "%s: view_stride = %d is below the n = %d clips of a view", who, view_stride, n);
    PC_CHECK_ARG(f_skip >= 1, "%s: f_skip = %d", who, f_skip);
    g.V = V; g.n = n; g.view_stride = view_stride; g.f_skip = f_skip;
    return PC_OK;
}

// views: int32 [g.V][3] = (h0, w0, flip)
inline int geom_views(ClipGeom& g, const char* who, const int32_t* views) {
    g.flips = 0;
    for (int v = 0; v < MAX_VIEWS; ++v) {
        g.vh0[v] = g.vw0[v] = 0;
        if (v >= g.V) continue;
        const int h0 = views[3 * v], w0 = views[3 * v + 1], fl = views[3 * v + 2];
        PC_CHECK_ARG(h0 >= 0 && w0 >= 0 && (int64_t)h0 + g.S <= g.H && (int64_t)w0 + g.S <= g.W, "%s: view %d, crop %d+%d x %d+%d outside %d x %d", who,
                     v, h0, g.S, w0, g.S, g.H, g.W);
        PC_CHECK_ARG(fl == 0 || fl == 1, "%s: view %d, flip = %d is neither 0 nor 1", who, v, fl);
        g.vh0[v] = h0; g.vw0[v] = w0; g.flips |= (uint32_t)fl << v;
    }
    return PC_OK;
}

// starts: int32 [g.n]
inline int geom_starts(ClipGeom& g, const char* who, const int32_t* starts) {
    for (int c = 0; c < MAX_CLIPS; ++c) {
        if (c < g.n) PC_CHECK_ARG(starts[c] >= 0, "%s: start %d of clip %d is negative", who, starts[c], c);
        g.starts[c] = c < g.n ? starts[c] : 0;
    }
    return PC_OK;
}
