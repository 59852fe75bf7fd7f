// Overlapping clips in time (detect.DetectEngine.set_clip_hop): the one statement of which windows a video is cut into and which of them
// hold a frame, shared by the host entry pc_clip_hop_starts and the kernels of cliphop.hip so that they cannot disagree.
//   span = 8 * f_skip frames per window; hop: a multiple of f_skip in [f_skip, span], the distance between two windows (hop == span: the
//   cut of evalstep.clip_starts, every frame in one window)
//   windows start at m * hop, m = 0 .. hop_windows - 1: the first one, and every further one whose predecessor does not reach the video's
//   end ((m - 1) * hop + span < F) -- no window holds more padding than necessary
//   clip starts are m * hop + j for the phases j = 0 .. f_skip - 1 with m * hop + j < F, in that order; the clip with start s has index
//   (s / hop) * f_skip + s % hop (s % hop < f_skip) -- but for the last window of a video whose phases run over its end, which is the last
//   of the list either way, so the index holds for every clip that exists
//   frame f lies in the windows hop_lo .. hop_hi (1 .. M = hop_slots <= 8 of them), in each of them in the clip of phase f % f_skip;
//   consecutive windows have pairwise distinct m % M, the plane slot of a window
// Everything is integer arithmetic on values below 2^31 in 64 bits.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PC_HOP_HD __host__ __device__ __forceinline__
#else
#define PC_HOP_HD inline
#endif

constexpr int HOP_MAX_F_SKIP = 1 << 20;                              // keeps span and every product of the rule far inside 32 bits

PC_HOP_HD bool hop_ok(int f_skip, int hop) {
    return f_skip >= 1 && f_skip <= HOP_MAX_F_SKIP && hop >= f_skip && hop <= 8 * f_skip && hop % f_skip == 0;
}

PC_HOP_HD int hop_slots(int f_skip, int hop) { return (8 * f_skip + hop - 1) / hop; }

PC_HOP_HD int64_t hop_windows(int64_t F, int f_skip, int hop) {
    const int64_t span = 8 * (int64_t)f_skip;
    return F <= span ? 1 : 1 + (F - span + hop - 1) / hop;
}

// first and last window that hold frame f < F
PC_HOP_HD int64_t hop_lo(int64_t f, int f_skip, int hop) {
    const int64_t a = f - 8 * (int64_t)f_skip + 1;
    return a <= 0 ? 0 : (a + hop - 1) / hop;
}

PC_HOP_HD int64_t hop_hi(int64_t F, int64_t f, int f_skip, int hop) {
    const int64_t a = f / hop, b = hop_windows(F, f_skip, hop) - 1;
    return a < b ? a : b;
}

// clips of the video: f_skip per window, fewer in a last window whose phases run over the end
PC_HOP_HD int64_t hop_clips(int64_t F, int f_skip, int hop) {
    const int64_t last = (hop_windows(F, f_skip, hop) - 1) * hop, left = F - last;
    return (hop_windows(F, f_skip, hop) - 1) * f_skip + (left < f_skip ? left : f_skip);
}
