// Device helpers shared by the kernels that walk uint8 maps [F][H][W] in four-pixel groups and count across a wave's lanes
// (instances.hip, maskruns.hip).
#pragma once
#include "common.h"

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// the set bits of a ballot in the lanes below this one
__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// bytes4: the four bytes at q, of which the first n (0..4) are wanted (the others hold whatever lies there); fg_bits: four pixels at q as bits
// 0..3 (non-zero byte = foreground), the first n of them count.  q itself must be a byte of the mask even for n = 0.  A frame starts at any
// byte address when W is odd, so the four bytes come out of the one or two ALIGNED dwords that hold them -- the second is fetched only if it holds one of the n bytes, so every dword read holds a byte of the mask and lies in its allocation -- and there is
// no branch around the loads: a caller's loads for several rows are all issued before the first is waited for.
__device__ __forceinline__ uint32_t bytes4(const uint8_t* q, int n) {
    const uintptr_t a = (uintptr_t)q;
    const int sh = (int)(a & 3);
    const uint32_t* p0 = (const uint32_t*)(a - sh);
    const uint32_t* p1 = (4 - sh < n) ? p0 + 1 : p0;
    const uint32_t w0 = *p0, w1 = *p1;
    return (uint32_t)((((unsigned long long)w1 << 32) | w0) >> (8 * sh));
}

__device__ __forceinline__ uint32_t fg_bits(const uint8_t* q, int n) {
    const uint32_t v = bytes4(q, n);
    const uint32_t b = ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 2u : 0u) | ((v & 0xff0000u) ? 4u : 0u) | ((v & 0xff000000u) ? 8u : 0u);
    return b & ((1u << n) - 1u);
}

// the four bytes themselves, the ones past the first n as zeros (a map value, not a bit)
__device__ __forceinline__ uint32_t map_bytes(const uint8_t* q, int n) {
    const uint32_t v = bytes4(q, n);
    return n >= 4 ? v : (v & ((1u << (8 * n)) - 1u));
}
