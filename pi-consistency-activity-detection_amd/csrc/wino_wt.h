// F(2x2, 3x3) weight transform of one (tap frame, output channel, input channel): the body of wino_weights_kernel, in a header so that
// the kernel that runs many weight-transform jobs of both Winograd forms in one launch (wino4.hip) executes the same instructions.
#pragma once
#include "common.h"

namespace {

// ---- weight transform: U[kt][ct][c8][xi*4+nu][kh][co 64][4] = (G g G^T)[xi][nu] of g = w[o][kt][.][.][i], read through strides so
// the master OIDHW tensor (forward) and its transpose with mirrored taps (input gradient) need no intermediate layout.
// One element e = (kt, o, i) of the transform, e < KT * nct * 64 * I (the caller checks): shared by wino_weights_kernel (wino.hip) and the
// many-jobs kernel (wino4.hip).
__device__ __forceinline__ void wino2_weights_elem(long long e, const float* __restrict__ w, long long sO, long long sT, long long sI, int O, int I, int KT, int flip,
                                                   float* __restrict__ U, int nct, int nc8) {
    const int i = (int)(e % I);
    long long r = e / I;
    const int o = (int)(r % (nct * 64));
    const int kt = (int)(r / (nct * 64));
    float g[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int ks = flip ? KT - 1 - kt : kt, as = flip ? 2 - a : a, bs = flip ? 2 - b : b;
            g[a][b] = o < O ? w[(long long)o * sO + (long long)((ks * 3 + as) * 3 + bs) * sT + (long long)i * sI] : 0.f;
        }
    float t[4][3];          // G g
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        t[0][b] = g[0][b];
        t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
        t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
        t[3][b] = g[2][b];
    }
    float* dst = U + ((((long long)kt * nct + o / 64) * nc8 + i / 8) * 16) * (2 * 64 * 4) + ((long long)((i & 7) >> 2) * 64 + (o & 63)) * 4 + (i & 3);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const float u0 = t[x][0], u1 = 0.5f * (t[x][0] + t[x][1] + t[x][2]), u2 = 0.5f * (t[x][0] - t[x][1] + t[x][2]), u3 = t[x][2];
        dst[(x * 4 + 0) * (2 * 64 * 4)] = u0;
        dst[(x * 4 + 1) * (2 * 64 * 4)] = u1;
        dst[(x * 4 + 2) * (2 * 64 * 4)] = u2;
        dst[(x * 4 + 3) * (2 * 64 * 4)] = u3;
    }
}

}  // namespace
