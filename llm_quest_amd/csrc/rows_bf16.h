// Packed-bf16 row helpers of the side kernels (qwen35.hip, hyper_conn.hip, decode.hip, gemma3.hip).
// elementwise.hip and norm_rope.hip keep copies of their own: their bytes are part of the step's source fingerprint
// (fingerprint.kernel_sources_sha); they become users the next time the counter evidence is re-collected anyway.
#pragma once
#include "common.h"

// 8 packed bf16 (16 bytes) <-> 8 floats
__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(v[e] << 16);
        f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
    }
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(f[2 * e], f[2 * e + 1]);
    return o;
}
__device__ __forceinline__ float rbf(float x) { return bf2f(f2bf(x)); }  // round through bf16
