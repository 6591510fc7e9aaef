// What the mixture-of-experts files (moe.hip, deepseek_moe.hip, latent_moe.hip) share and nobody else uses: the E / k limits, the host checks of their entry
// points, the two ends of a router kernel (the token's softmax in front of the selection, the write-out behind it), the bias-balanced selection between them
// (deepseek_moe.hip and latent_moe.hip) and the declaration of the one combine launcher.  Internal: not installed, no entry point lives here.
#pragma once
#include <initializer_list>

#include "host_checks.h"
#include "rows_bf16.h"

constexpr int MOE_MAX_E = 128;  // two experts per lane in the route kernels
constexpr int MOE_MAX_K = 8;

// out[t] = residual[t] + (shared[t] + sum_j w[t, j] * Y[slot[t, j]]); w, shared and residual may each be null.  Validates, launches the one combine
// kernel (moe.hip) and reports under the entry point's name ``who``.
int moe_combine_fwd_launch(const char* who, int64_t T, int64_t R, int k, int d, const int32_t* slot, const void* w, const void* y, int64_t ldy, const void* shared,
                           int64_t lds, const void* residual, int64_t ldr, void* out, int64_t ldo, void* stream);

namespace {

__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// ------------------------------------------------------------------------------------------------ the two ends of a router kernel
// One wave per token; lane l holds experts l and l + 64.  pb = bf16(softmax(row)) (0 beyond E; columns at and beyond E are never read).
__device__ __forceinline__ void route_softmax(const bf16_t* __restrict__ row, int E, int lane, bf16_t (&pb)[2]) {
    float x[2], e[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) x[h] = lane + 64 * h < E ? bf2f(row[lane + 64 * h]) : -INFINITY;
    const float m = wave_max(fmaxf(x[0], x[1]));
#pragma unroll
    for (int h = 0; h < 2; ++h) e[h] = lane + 64 * h < E ? expf(x[h] - m) : 0.f;
    const float den = wave_sum(e[0] + e[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) pb[h] = f2bf(e[h] / den);
}

// s = bf16(sum_j v_j) (``sum``: the v_j added in slot order), idx_j = ex_j, w_j = bf16(v_j / s): lane 0 writes the token's row
__device__ __forceinline__ void route_write(int64_t t, int k, int lane, const int (&ex)[MOE_MAX_K], const float (&v)[MOE_MAX_K], float sum, int* __restrict__ idx,
                                            bf16_t* __restrict__ w, float* __restrict__ s) {
    const float sr = rbf(sum);
    if (lane == 0) {
        s[t] = sr;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                idx[t * k + j] = ex[j];
                w[t * k + j] = f2bf(v[j] / sr);
            }
    }
}

// ------------------------------------------------------------------------------------------------ the bias-balanced selection (DeepSeekMoE, LatentMoE)
__device__ __forceinline__ unsigned wave_umin(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned u = (unsigned)__shfl_xor((int)v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}

// fp32 bits -> an unsigned that orders like the value; never 0 for a number (0 marks a lane that holds no live expert)
__device__ __forceinline__ unsigned order_f32(float x) {
    const unsigned b = __float_as_uint(x);
    const unsigned o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return o == 0u ? 1u : o;
}

// the lane's two balancing biases as floats (0 beyond E)
template <bool BIAS_F32>
__device__ __forceinline__ void route_load_bias(const void* __restrict__ bias, int E, int lane, float (&bv)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        bv[h] = 0.f;
        if (lane + 64 * h < E) bv[h] = BIAS_F32 ? ((const float*)bias)[lane + 64 * h] : bf2f(((const bf16_t*)bias)[lane + 64 * h]);
    }
}

// Between a token's bf16 probabilities pf (as floats, 0 beyond E) and the write-out: the k experts ex_j and their UNBIASED probabilities v_j; returns their sum in
// slot order.  The key is pf + bv in the promoted dtype of p and the buffer (a bf16 sum, or fp32 with BIAS_F32); k rounds of a wave maximum over the keys and a wave
// minimum over the experts that hold it: the lowest expert among equal keys, and k <= E keeps one alive.  FORCED: the token's row of given experts instead
// (``forced``: its k entries); one that is no expert weighs 0, and mi355_moe_plan gives the assignment no row.
template <bool BIAS_F32, bool FORCED>
__device__ __forceinline__ float route_select_biased(const float (&pf)[2], const float (&bv)[2], const int* __restrict__ forced, int E, int k, int lane,
                                                     int (&ex)[MOE_MAX_K], float (&v)[MOE_MAX_K]) {
    float sum = 0.f;
    if (FORCED) {
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                const int f = forced[j];
                const bool ok = f >= 0 && f < E;
                const float lo = __shfl(pf[0], ok ? (f & 63) : 0, 64), hi = __shfl(pf[1], ok ? (f & 63) : 0, 64);
                ex[j] = f;
                v[j] = ok ? (f >= 64 ? hi : lo) : 0.f;
                sum += v[j];
            }
    } else {
        unsigned key[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float kf = BIAS_F32 ? pf[h] + bv[h] : rbf(pf[h] + bv[h]);
            key[h] = lane + 64 * h < E ? order_f32(kf) : 0u;
        }
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                const unsigned best = wave_umax(key[0] > key[1] ? key[0] : key[1]);
                const unsigned mine = (key[0] != 0u && key[0] == best) ? (unsigned)lane : ((key[1] != 0u && key[1] == best) ? (unsigned)(lane + 64) : 255u);
                const int sel = (int)wave_umin(mine);
                const float lo = __shfl(pf[0], sel & 63, 64), hi = __shfl(pf[1], sel & 63, 64);
                ex[j] = sel;
                v[j] = sel >= 64 ? hi : lo;
                sum += v[j];  // slot order
                if (sel == lane) key[0] = 0u;
                if (sel == lane + 64) key[1] = 0u;
            }
    }
    return sum;
}

inline bool bias_dtype_ok(int dt) { return dt == MI355_DT_BF16 || dt == MI355_DT_F32; }

// ------------------------------------------------------------------------------------------------ host checks
inline int capped_grid(int64_t blocks) { return (int)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)); }

// 1 <= k <= 8, k <= E <= 128, T * k + 64 * E < 2^31
inline int check_route(const char* who, int64_t T, int E, int k) {
    MI355_REQUIRE(E >= 1 && E <= MOE_MAX_E, "%s: num_experts (the routed experts) must be in 1..%d (got %d)", who, MOE_MAX_E, E);
    MI355_REQUIRE(k >= 1 && k <= MOE_MAX_K && k <= E, "%s: top_k must be in 1..%d and at most num_experts = %d (got %d)", who, MOE_MAX_K, E, k);
    MI355_REQUIRE(T < (int64_t)1 << 31 && T * k + 64 * (int64_t)E < (int64_t)1 << 31, "%s: tokens * top_k + 64 * num_experts must stay below 2^31 (tokens = %ld)", who,
                  (long)T);
    return 0;
}

// ``rows`` rows of width d behind each of the leading dimensions
inline int check_rows(const char* who, int64_t rows, int d, std::initializer_list<int64_t> lds) {
    MI355_REQUIRE(rows < (int64_t)1 << 31, "%s: row counts must stay below 2^31 (got %ld)", who, (long)rows);
    MI355_REQUIRE(d > 0 && (d & 7) == 0, "%s: the row width must be a positive multiple of 8 (got %d)", who, d);
    for (int64_t ld : lds) MI355_REQUIRE(ld >= d && (ld & 7) == 0, "%s: a leading dimension must be a multiple of 8 and at least the row width %d (got %ld)", who, d, (long)ld);
    return 0;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
