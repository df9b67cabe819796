// Stored samples -> the network's fp32: what the per-batch gather (k_batch.hip) and the scene gather (k_scene.hip) share, so that both
// produce the same bits for the same samples.  Device code only.
#pragma once
#include "common.h"

template <typename T> struct Vec16 { static constexpr int N = 16 / (int)sizeof(T); };

// the 16 bytes of one load as Vec16<T>::N floats
__device__ __forceinline__ void unpack16(const uint4& r, float (&f)[16], const uint8_t*) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = (float)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
}
__device__ __forceinline__ void unpack16(const uint4& r, float (&f)[8], const uint16_t*) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)((w[i >> 1] >> (16 * (i & 1))) & 0xffffu);
}
__device__ __forceinline__ void unpack16(const uint4& r, float (&f)[4], const float*) {
    f[0] = __uint_as_float(r.x); f[1] = __uint_as_float(r.y); f[2] = __uint_as_float(r.z); f[3] = __uint_as_float(r.w);
}

__device__ __forceinline__ float ba_scale(float x, float divisor, int n_div, float post_scale, int has_scale) {
    if (n_div > 0) x = __fdiv_rn(x, divisor);
    if (n_div > 1) x = __fdiv_rn(x, divisor);
    if (has_scale) x = __fmul_rn(x, post_scale);
    return x;
}
