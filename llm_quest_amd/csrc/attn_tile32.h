// The plain 32-key tile layer of attention_generic.hip, attention_band.hip, deepseek.hip and llama3.hip's max-logit kernel: padded, unswizzled
// LDS images of 32 rows x D bf16, the MFMA operand fragments read from them (mfma_f32_32x32x16_bf16, the transposed one through
// ds_read_b64_tr_b16), the steps of one tile (score product, online-softmax update, transposed accumulate), the write-out of a transposed
// accumulator, and the delta kernel of the backward.  Not the layer of attention.hip: attn_common.h has its own swizzled, DMA-fed frag_rows /
// frag_cols / pack_frag under the same names, so a translation unit includes one of the two headers, never both.
#pragma once
#include "common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
#define NEG_INF (-__builtin_huge_valf())

template <int D>
struct Tile32 {
    static constexpr int PITCH = D * 2 + 16;  // bytes per LDS row
    static constexpr int KS = D / 16;         // k-steps over d
    static constexpr int DT = D / 32;         // 32-row tiles of a transposed [d x 32] accumulator
    static constexpr int IMG = 32 * PITCH;    // one 32-row image
};

// cooperative load by NT threads of 32 rows x D bf16 (rows base, base + ld, ..) into a padded LDS image; rows >= rows_valid are zero
template <int D, int NT>
__device__ __forceinline__ void load_tile(char* img, const bf16_t* base, int64_t ld, int rows_valid, int tid) {
    constexpr int CH = D / 8;
    for (int c = tid; c < 32 * CH; c += NT) {
        const int row = c / CH, ch = c % CH;
        u32x4 v = {0, 0, 0, 0};
        if (row < rows_valid) v = *reinterpret_cast<const u32x4*>(base + (int64_t)row * ld + ch * 8);
        *reinterpret_cast<u32x4*>(img + row * Tile32<D>::PITCH + ch * 16) = v;
    }
}
// A operand (32 rows x 16 k) from a row image: row = lane & 31, k = 16 ks + 8 (lane >> 5) ..
template <int D>
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(img + (lane & 31) * Tile32<D>::PITCH + (2 * ks + (lane >> 5)) * 16);
}
// A operand of the TRANSPOSE of a row image: rows of A = image columns c0 .. c0+31, k = image rows in the order in which an
// accumulator tile packs into a B operand: element j <-> image row k0 + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)
template <int D>
__device__ __forceinline__ bf16x8 frag_cols(const char* img, int c0, int k0, int lane) {
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p = lane & 3;
    const int row = k0 + 4 * (g >> 1) + q4;
    const int col = c0 + 16 * (g & 1) + 4 * p;
    const char* a = img + row * Tile32<D>::PITCH + col * 2;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(a));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(a + 8 * Tile32<D>::PITCH));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ bf16x8 pack_frag(const f32x16& x, int s) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(x[8 * s + 2 * e], x[8 * s + 2 * e + 1]);
    return __builtin_bit_cast(bf16x8, o);
}
// B operand fragments of a row held on the lane (row = lane & 31 of the wave's 32 rows)
template <int D>
__device__ __forceinline__ void load_row_frags(const bf16_t* rowptr, bool valid, int lane, bf16x8 (&f)[Tile32<D>::KS]) {
#pragma unroll
    for (int ks = 0; ks < Tile32<D>::KS; ++ks) {
        u32x4 v = {0, 0, 0, 0};
        if (valid) v = *reinterpret_cast<const u32x4*>(rowptr + 16 * ks + 8 * (lane >> 5));
        f[ks] = __builtin_bit_cast(bf16x8, v);
    }
}

// ---- the steps of one 32-key tile, as every kernel on this layer takes them.  Each family keeps its own mask, tile range and write-out.
// the image row (key of a score tile S^T, query in the key-major pass) that element i of a lane's accumulator tile belongs to
__device__ __forceinline__ int acc_row(int i, int lane) { return 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3); }
__device__ __forceinline__ void zero_tile(f32x16& t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = 0.f;
}
template <int N>
__device__ __forceinline__ void zero_tiles(f32x16 (&t)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) zero_tile(t[n]);
}
// t += (32 image rows x D) . (the D features of the row held on the lane): a score tile S^T = K Q^T, or dP^T = V dO^T
template <int D>
__device__ __forceinline__ void mma_rows(f32x16& t, const char* img, const bf16x8 (&f)[Tile32<D>::KS], int lane) {
#pragma unroll
    for (int ks = 0; ks < Tile32<D>::KS; ++ks) t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(img, ks, lane), f[ks], t, 0, 0, 0);
}
// t += (image columns c0 .. c0+31 of a D-wide image)^T . P^T, P^T packed from an accumulator tile as p0 = pack_frag(., 0), p1 = pack_frag(., 1)
template <int D>
__device__ __forceinline__ void mma_cols(f32x16& t, const char* img, int c0, const bf16x8& p0, const bf16x8& p1, int lane) {
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(img, c0, 0, lane), p0, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(img, c0, 16, lane), p1, t, 0, 0, 0);
}
// The online-softmax update of a row's state (m, l, acc) with one tile of masked scores (log2 units, NEG_INF where masked) and mx, the largest
// of the lane's 16 (the caller's mask loop keeps it): s becomes exp2(s - m).  m_use: a row no tile has reached yet (a window that starts
// later, a row past S) keeps m = -inf and adds nothing.
template <int N>
__device__ __forceinline__ void online_softmax(f32x16& s, float mx, float& m, float& l, f32x16 (&acc)[N]) {
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float m_use = m_new == NEG_INF ? 0.f : m_new;
    const float alpha = exp2f(m - m_use);
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        s[i] = exp2f(s[i] - m_use);
        rs += s[i];
    }
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
    m = m_new;
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[n][i] *= alpha;
}

// accumulator tile [32 d x 32 rows-on-lane] -> token-major bf16 rows (4 consecutive d per 8-byte store)
template <int NDT>
__device__ __forceinline__ void store_t_tiles(const f32x16 (&acc)[NDT], float mul, bf16_t* rowptr, bool valid, int lane) {
    if (!valid) return;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i4 = 0; i4 < 4; ++i4) {
            u32x2 w;
            w[0] = pack_bf2(acc[dt][4 * i4] * mul, acc[dt][4 * i4 + 1] * mul);
            w[1] = pack_bf2(acc[dt][4 * i4 + 2] * mul, acc[dt][4 * i4 + 3] * mul);
            *reinterpret_cast<u32x2*>(rowptr + 32 * dt + 8 * i4 + 4 * (lane >> 5)) = w;
        }
}

// delta[b, h, s] = sum_d dO * O.  A non-template kernel in a header: the anonymous namespace gives every including translation unit its own.
__global__ __launch_bounds__(256) void attn_delta_kernel(int64_t tokens, int S, int Hq, int D, const bf16_t* __restrict__ o, int64_t ldo,
                                                         const bf16_t* __restrict__ d_o, int64_t lddo, float* __restrict__ delta) {
    const int lane = threadIdx.x & 63;
    const int64_t total = tokens * Hq;
    for (int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); item < total; item += (int64_t)gridDim.x * 4) {
        const int64_t t = item / Hq;
        const int h = (int)(item % Hq);
        float acc = 0.f;
        for (int i = lane; i < D; i += 64) acc += bf2f(o[t * ldo + (int64_t)h * D + i]) * bf2f(d_o[t * lddo + (int64_t)h * D + i]);
        acc = wave_sum(acc);
        if (lane == 0) delta[((t / S) * Hq + h) * S + (t % S)] = acc;
    }
}

}  // namespace
