// How the kernels that walk a uint16 probability map [F][H][W] in four-pixel groups (probhist.hip, probcut.hip) fetch a group, said once.
#pragma once
#include "common.h"

// the four probabilities at q (the first n of them wanted, the others 0) as two dwords; wide: q is 8-byte aligned
__device__ __forceinline__ uint2 prob_words(const uint16_t* q, int n, bool wide) {
    if (wide && n == 4) return *(const uint2*)q;
    uint32_t v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < n ? (uint32_t)q[e] : 0u;
    return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}
