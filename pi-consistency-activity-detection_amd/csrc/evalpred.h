// Decisions the evaluator and the detection output share, so that a detection and its score can never disagree:
//   seg_positive       the evaluator's mask predicate, fp32 sigmoid(x) >= 0.5 (evaluate_ucf101.py:128)
//   vote_mean_argmax   np.argmax(np.mean(predictions, axis=0)) (evaluate_ucf101.py:139-146)
#pragma once
#include "common.h"

// sigmoid(x) >= 0.5 in fp32: certainly true for x >= 0 (exp(-x) <= 1 => 1 + e <= 2, division is monotone) and certainly false below -1e-6
// (1 + e >= 2.000001 > 2); only in between does the rounding of exp / the sum decide.  A NaN fails all three comparisons: background.
__device__ __forceinline__ bool seg_positive(float x) {
    return x >= 0.f ? true : (x < -1e-6f ? false : (1.0f / (1.0f + expf(-x))) >= 0.5f);
}

__device__ __forceinline__ bool vote_better(float a, int ia, float b, int ib) {     // np.argmax: the first maximum; a NaN beats every number
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ia < ib;
}

// One block of 256 threads: the n rows of pred [n][C] added in row order in fp32 and divided once by (float)n, as numpy's mean over axis 0
// of a C-contiguous float32 array; the means go to `means` [C] if it is not null.  bv / bi: 256 words of LDS each.  Holds a block barrier:
// every thread of the block calls it.  Thread 0 returns (arg-max, mean at the arg-max) in best / besti; the other threads' are partial.
__device__ __forceinline__ void vote_mean_argmax(const float* __restrict__ pred, int n, int C, float* __restrict__ means, float* bv, int* bi,
                                                 float& best, int& besti) {
    best = 0.f; besti = 0x7fffffff;
    for (int j = threadIdx.x; j < C; j += 256) {
        float s = pred[j];
        for (int r = 1; r < n; ++r) s = __fadd_rn(s, pred[(size_t)r * C + j]);
        const float m = __fdiv_rn(s, (float)n);
        if (means) means[j] = m;
        if (besti == 0x7fffffff || vote_better(m, j, best, besti)) { best = m; besti = j; }
    }
    bv[threadIdx.x] = best; bi[threadIdx.x] = besti;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int live = C < 256 ? C : 256;
        for (int t = 1; t < live; ++t)
            if (vote_better(bv[t], bi[t], best, besti)) { best = bv[t]; besti = bi[t]; }
    }
}
