// Preference tuning (alignment/dpo/dpo.py, alignment/rlhf_grpo/grpo_engine.py: PrefRewardCalculator): the arithmetic that is left around the label
// log-prob kernels (grpo.hip, grpo_head.hip) in a DPO step and around a backbone's hidden states in a reward model.  Three families:
//   * the masked sequence average of DPOLoss.compute_logprobs over fp32 log-probs [B, T] and its backward,
//   * the DPO loss of a batch: the loss, the two reward means and both policy gradients from one launch,
//   * the reward pooling of PrefRewardCalculator in four modes, one pass over the hidden states in 16-byte loads, and its backward.
// fp32 arithmetic, the sums of a sequence or of the batch in fp64 where they end in one number; every reduction has a fixed order (per thread
// ascending, the lanes by the xor tree, the four waves in order); no atomics anywhere: two runs give the same bits.
#include <math.h>

#include "rows_bf16.h"

namespace {

enum { M_U8 = 0, M_I32 = 1, M_I64 = 2, M_F32 = 3, M_BF16 = 4 };                                  // the mask dtype codes of grpo.hip
enum { POOL_SCORES = 0, POOL_HIDDEN_MEAN = 1, POOL_LAST_TOKEN = 2, POOL_SCORES_FROM_HIDDEN = 3 };  // the modes of mi355_reward_pool_*
enum { D_BF16 = 0, D_F32 = 1 };                                                                  // MI355_DT_*

__device__ __forceinline__ float pref_mask_at(const void* mask, int dt, int64_t i) {
    switch (dt) {
        case M_U8: return ((const uint8_t*)mask)[i] ? 1.f : 0.f;
        case M_I32: return (float)((const int32_t*)mask)[i];
        case M_I64: return (float)((const int64_t*)mask)[i];
        case M_F32: return ((const float*)mask)[i];
        default: return bf2f(((const bf16_t*)mask)[i]);
    }
}

__device__ __forceinline__ double pref_block_sum(double v, double* red) {  // 256 threads; red: 4 doubles of LDS
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float pref_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// 8 consecutive elements of a bf16 or fp32 row as floats (16-byte loads), and the store of 8 floats in either type
__device__ __forceinline__ void load8(const void* p, int dt, int64_t i, float (&f)[8]) {
    if (dt == D_BF16) {
        unpack8(*(const u32x4*)((const bf16_t*)p + i), f);
    } else {
        const f32x4 a = *(const f32x4*)((const float*)p + i), b = *(const f32x4*)((const float*)p + i + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = a[e], f[4 + e] = b[e];
    }
}
__device__ __forceinline__ void store8(void* p, int dt, int64_t i, const float (&f)[8]) {
    if (dt == D_BF16) {
        *(u32x4*)((bf16_t*)p + i) = pack8(f);
    } else {
        const f32x4 a = {f[0], f[1], f[2], f[3]}, b = {f[4], f[5], f[6], f[7]};
        *(f32x4*)((float*)p + i) = a;
        *(f32x4*)((float*)p + i + 4) = b;
    }
}
__device__ __forceinline__ float load1(const void* p, int dt, int64_t i) { return dt == D_BF16 ? bf2f(((const bf16_t*)p)[i]) : ((const float*)p)[i]; }
__device__ __forceinline__ void store1(void* p, int dt, int64_t i, float v) {
    if (dt == D_BF16) ((bf16_t*)p)[i] = f2bf(v);
    else ((float*)p)[i] = v;
}

// ------------------------------------------------------------------------------------------- the sequence average of compute_logprobs
// One workgroup per sequence.  avg[b] = sum_t logp[b, t] mask[b, t + 1] / sum_s mask[b, s], the denominator over all T + 1 positions and not clamped
// (an all-zero mask: 0 / 0, NaN, as upstream); without a mask the mean over the T labels.  den[b] is kept for the backward.
__global__ __launch_bounds__(256) void dpo_seq_logprob_kernel(int64_t T, const float* __restrict__ logp, const void* __restrict__ mask, int mdt,
                                                              float* __restrict__ avg, float* __restrict__ den) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int64_t o = (int64_t)b * T, om = (int64_t)b * (T + 1);
    double num = 0.0, d = 0.0;
    if (mask) {
        for (int64_t t = threadIdx.x; t < T; t += 256) num += (double)(logp[o + t] * pref_mask_at(mask, mdt, om + t + 1));
        for (int64_t s = threadIdx.x; s <= T; s += 256) d += (double)pref_mask_at(mask, mdt, om + s);
        d = pref_block_sum(d, red);
    } else {
        for (int64_t t = threadIdx.x; t < T; t += 256) num += (double)logp[o + t];
        d = (double)T;
    }
    num = pref_block_sum(num, red);
    if (threadIdx.x == 0) {
        avg[b] = (float)(num / d);
        den[b] = (float)d;
    }
}
// dlogp[b, t] = g[b] mask[b, t + 1] / den[b]
__global__ __launch_bounds__(256) void dpo_seq_logprob_bwd_kernel(int64_t T, const float* __restrict__ g, const void* __restrict__ mask, int mdt,
                                                                  const float* __restrict__ den, float* __restrict__ dlogp) {
    const int b = blockIdx.x;
    const int64_t o = (int64_t)b * T, om = (int64_t)b * (T + 1);
    const float gb = g[b], db = den[b];
    for (int64_t t = threadIdx.x; t < T; t += 256) dlogp[o + t] = (mask ? gb * pref_mask_at(mask, mdt, om + t + 1) : gb) / db;
}

// ------------------------------------------------------------------------------------------- the DPO loss
// log sigmoid(x) = min(x, 0) - log1p(exp(-|x|)) and sigmoid(x) without an overflow at either end
__device__ __forceinline__ float log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_stable(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
// One workgroup.  l = (pc - rc) - (pr - rr);  losses = -logsigmoid(beta l) (1 - ls) - logsigmoid(-beta l) ls;  out = [mean losses, mean(pc - rc),
// mean(pr - rr)] (the rewards are not scaled by beta);  dpc = d out[0] / d pc = beta (ls sigmoid(beta l) - (1 - ls) sigmoid(-beta l)) / n,  dpr = -dpc.
__global__ __launch_bounds__(256) void dpo_loss_kernel(int n, const float* __restrict__ pc, const float* __restrict__ pr, const float* __restrict__ rc,
                                                       const float* __restrict__ rr, float beta, float ls, float* __restrict__ out,
                                                       float* __restrict__ dpc, float* __restrict__ dpr) {
    __shared__ double red[4];
    double sl = 0.0, sc = 0.0, sr = 0.0;
    const float inv_n = 1.f / (float)n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float c = pc[i] - rc[i], r = pr[i] - rr[i];
        const float x = beta * (c - r);
        sl += (double)(-log_sigmoid(x) * (1.f - ls) - log_sigmoid(-x) * ls);
        sc += (double)c;
        sr += (double)r;
        const float d = beta * (ls * sigmoid_stable(x) - (1.f - ls) * sigmoid_stable(-x)) * inv_n;
        if (dpc) dpc[i] = d;
        if (dpr) dpr[i] = -d;
    }
    sl = pref_block_sum(sl, red);
    sc = pref_block_sum(sc, red);
    sr = pref_block_sum(sr, red);
    if (threadIdx.x == 0) {
        out[0] = (float)(sl / (double)n);
        out[1] = (float)(sc / (double)n);
        out[2] = (float)(sr / (double)n);
    }
}

// ------------------------------------------------------------------------------------------- reward pooling
// scores_mean_pooling on the head's output [B, S] (the (b, s, 1) rewards): one workgroup per sequence.  Positions whose mask is 0 are not read.
__global__ __launch_bounds__(256) void reward_scores_fwd_kernel(int64_t S, const void* __restrict__ x, int xdt, const void* __restrict__ mask, int mdt,
                                                                float* __restrict__ score, float* __restrict__ cnt) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int64_t o = (int64_t)b * S;
    double num = 0.0, c = 0.0;
    for (int64_t s = threadIdx.x; s < S; s += 256) {
        const float m = pref_mask_at(mask, mdt, o + s);
        if (m != 0.f) {
            num += (double)(load1(x, xdt, o + s) * m);
            c += (double)m;
        }
    }
    num = pref_block_sum(num, red);
    c = pref_block_sum(c, red);
    if (threadIdx.x == 0) {
        score[b] = (float)(num / fmax(c, 1.0));
        cnt[b] = (float)c;
    }
}
__global__ __launch_bounds__(256) void reward_scores_bwd_kernel(int64_t S, const float* __restrict__ g, const void* __restrict__ mask, int mdt,
                                                                const float* __restrict__ cnt, void* __restrict__ dx, int xdt) {
    const int b = blockIdx.x;
    const int64_t o = (int64_t)b * S;
    const float w = g[b] / fmaxf(cnt[b], 1.f);
    for (int64_t s = threadIdx.x; s < S; s += 256) {
        const float m = pref_mask_at(mask, mdt, o + s);
        store1(dx, xdt, o + s, m != 0.f ? w * m : 0.f);
    }
}

// The row the last-token score reads: count - 1, a count of 0 selecting row S - 1 (upstream's index -1); kept inside [0, S).
__device__ __forceinline__ int64_t last_row(float cnt, int64_t S) {
    const int64_t r = (int64_t)cnt - 1;
    return r < 0 || r >= S ? S - 1 : r;
}

// The three modes on hidden states [B, S, E] (E a multiple of 8, at most 8 192): one workgroup of 256 threads per sequence.  E / 8 chunks of 16 bytes
// (bf16; two loads in fp32); CP = the chunk count rounded up to a power of two (at most 256) lanes sit side by side on a row, and the 256 / CP groups of
// lanes take the positions s = j, j + 256 / CP, ... ascending; a thread owns chunks c, c + 256, ... (at most four).  The groups' partial rows are
// added in group order through LDS.  pooled[b, :] = sum_s mask h / max(count, 1) (last token: the selected row), fp32, which the backward needs
// for the weight gradient;  score = pooled . w + bias (scores-from-hidden: the bias only where the count is positive).
__global__ __launch_bounds__(256) void reward_pool_fwd_kernel(int mode, int64_t S, int E, const void* __restrict__ x, int xdt,
                                                              const void* __restrict__ mask, int mdt, const void* __restrict__ w, int wdt,
                                                              const void* __restrict__ bias, float* __restrict__ score,
                                                              float* __restrict__ pooled, float* __restrict__ cnt) {
    __shared__ float part[256 * 8];
    __shared__ double redd[4];
    __shared__ float redf[4];
    const int b = blockIdx.x, C = E >> 3;
    int CP = 1;
    while (CP < C && CP < 256) CP <<= 1;
    const int NS = 256 / CP, c0 = threadIdx.x % CP, j = threadIdx.x / CP;
    const int64_t om = (int64_t)b * S, ox = (int64_t)b * S * E;
    double cd = 0.0;
    for (int64_t s = threadIdx.x; s < S; s += 256) cd += (double)pref_mask_at(mask, mdt, om + s);
    const float count = (float)pref_block_sum(cd, redd);
    float acc[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
    if (mode == POOL_LAST_TOKEN) {
        const int64_t row = last_row(count, S);
        if (j == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + k * 256;
                if (c < C) load8(x, xdt, ox + row * E + (int64_t)c * 8, acc[k]);
            }
        }
    } else {
        for (int64_t s = j; s < S; s += NS) {
            const float m = pref_mask_at(mask, mdt, om + s);
            if (m == 0.f) continue;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + k * 256;
                if (c < C) {
                    float f[8];
                    load8(x, xdt, ox + s * E + (int64_t)c * 8, f);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[k][e] += f[e] * m;
                }
            }
        }
        if (NS > 1) {  // C <= 128: one chunk per thread; fold the groups in order
#pragma unroll
            for (int e = 0; e < 8; ++e) part[threadIdx.x * 8 + e] = acc[0][e];
            __syncthreads();
            if (j == 0) {
                for (int g = 1; g < NS; ++g)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[0][e] += part[(g * CP + c0) * 8 + e];
            }
        }
        const float inv = 1.f / fmaxf(count, 1.f);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[k][e] *= inv;
    }
    float dot = 0.f;
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k * 256;
            if (c < C) {
                float wv[8];
                load8(w, wdt, (int64_t)c * 8, wv);
#pragma unroll
                for (int e = 0; e < 8; ++e) dot += acc[k][e] * wv[e];
                store8(pooled, D_F32, (int64_t)b * E + (int64_t)c * 8, acc[k]);
            }
        }
    }
    dot = pref_block_sum(dot, redf);
    if (threadIdx.x == 0) {
        float bv = bias ? load1(bias, wdt, 0) : 0.f;
        if (mode == POOL_SCORES_FROM_HIDDEN && !(count > 0.f)) bv = 0.f;
        score[b] = dot + bv;
        cnt[b] = count;
    }
}

// dhidden: a thread per 16-byte chunk of [B, S, E], grid-stride.  Hidden-mean and scores-from-hidden: g[b] mask / max(count, 1) times w; last token: g[b] w on
// the selected row.  Every other row is exact zeros.
__global__ __launch_bounds__(256) void reward_pool_dx_kernel(int mode, int64_t chunks, int64_t S, int E, const float* __restrict__ g,
                                                             const void* __restrict__ mask, int mdt, const float* __restrict__ cnt,
                                                             const void* __restrict__ w, int wdt, void* __restrict__ dx, int xdt) {
    const int C = E >> 3;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / C;
        const int c = (int)(i - row * C);
        const int64_t b = row / S, s = row - b * S;
        float coef;
        bool live;
        if (mode == POOL_LAST_TOKEN) {
            live = s == last_row(cnt[b], S);
            coef = g[b];
        } else {
            const float m = pref_mask_at(mask, mdt, row);
            live = m != 0.f;
            coef = g[b] * m / fmaxf(cnt[b], 1.f);
        }
        float f[8];
        if (live) {
            load8(w, wdt, (int64_t)c * 8, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= coef;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = 0.f;
        }
        store8(dx, xdt, i * 8, f);
    }
}
// dw[e] = sum_b g[b] pooled[b, e], b ascending, a thread per element;  dbias = sum_b g[b] (scores-from-hidden: over the sequences with a positive count)
__global__ __launch_bounds__(256) void reward_pool_dw_kernel(int mode, int B, int E, const float* __restrict__ g, const float* __restrict__ cnt,
                                                             const float* __restrict__ pooled, void* __restrict__ dw, void* __restrict__ dbias, int wdt) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (dw && e < E) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += g[b] * pooled[(int64_t)b * E + e];
        store1(dw, wdt, e, s);
    }
    if (dbias && e == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b)
            if (mode != POOL_SCORES_FROM_HIDDEN || cnt[b] > 0.f) s += g[b];
        store1(dbias, wdt, 0, s);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool mask_dtype_ok(int dt) { return dt >= M_U8 && dt <= M_BF16; }
bool dt_ok(int dt) { return dt == D_BF16 || dt == D_F32; }

}  // namespace

#define STREAM ((hipStream_t)stream)
#define MAX_T ((int64_t)1 << 31)

extern "C" int mi355_dpo_seq_logprob(int B, int64_t T, const float* logp, const void* mask, int mask_dtype, float* avg, float* den, void* stream) {
    MI355_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= MAX_T && logp && avg && den,
                  "mi355_dpo_seq_logprob: bad arguments (B in 1..65535, T in 1..2^31, non-null pointers; the mask alone may be NULL)");
    MI355_REQUIRE(!mask || mask_dtype_ok(mask_dtype), "mi355_dpo_seq_logprob: unknown mask dtype %d (0 u8 / bool, 1 i32, 2 i64, 3 f32, 4 bf16)", mask_dtype);
    hipLaunchKernelGGL(dpo_seq_logprob_kernel, dim3(B), dim3(256), 0, STREAM, T, logp, mask, mask_dtype, avg, den);
    MI355_LAUNCH_CHECK("mi355_dpo_seq_logprob");
    return 0;
}

extern "C" int mi355_dpo_seq_logprob_bwd(int B, int64_t T, const float* g, const void* mask, int mask_dtype, const float* den, float* dlogp,
                                         void* stream) {
    MI355_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= MAX_T && g && den && dlogp,
                  "mi355_dpo_seq_logprob_bwd: bad arguments (B in 1..65535, T in 1..2^31, non-null pointers; the mask alone may be NULL)");
    MI355_REQUIRE(!mask || mask_dtype_ok(mask_dtype), "mi355_dpo_seq_logprob_bwd: unknown mask dtype %d (0 u8 / bool, 1 i32, 2 i64, 3 f32, 4 bf16)", mask_dtype);
    hipLaunchKernelGGL(dpo_seq_logprob_bwd_kernel, dim3(B), dim3(256), 0, STREAM, T, g, mask, mask_dtype, den, dlogp);
    MI355_LAUNCH_CHECK("mi355_dpo_seq_logprob_bwd");
    return 0;
}

extern "C" int mi355_dpo_loss(int n, const float* pol_chosen, const float* pol_rejected, const float* ref_chosen, const float* ref_rejected, float beta,
                              float label_smoothing, float* out, float* dpol_chosen, float* dpol_rejected, void* stream) {
    MI355_REQUIRE(n > 0 && n <= (1 << 24) && pol_chosen && pol_rejected && ref_chosen && ref_rejected && out,
                  "mi355_dpo_loss: bad arguments (n in 1..2^24, non-null pointers; the two gradients alone may be NULL)");
    MI355_REQUIRE(beta == beta && label_smoothing == label_smoothing, "mi355_dpo_loss: beta and label_smoothing must be numbers");
    hipLaunchKernelGGL(dpo_loss_kernel, dim3(1), dim3(256), 0, STREAM, n, pol_chosen, pol_rejected, ref_chosen, ref_rejected, beta, label_smoothing, out,
                       dpol_chosen, dpol_rejected);
    MI355_LAUNCH_CHECK("mi355_dpo_loss");
    return 0;
}

static bool reward_pool_ok(const char* name, int mode, int B, int64_t S, int E, const void* mask, int mask_dtype, int x_dtype, const void* w,
                           int w_dtype) {
    if (!(mode >= POOL_SCORES && mode <= POOL_SCORES_FROM_HIDDEN)) {
        mi355_set_error("%s: unknown mode %d (0 scores mean, 1 hidden-state mean, 2 last token, 3 scores mean from hidden states)", name, mode);
        return false;
    }
    if (!(B > 0 && B <= 65535 && S > 0 && S <= MAX_T && mask)) {
        mi355_set_error("%s: bad arguments (B in 1..65535, S in 1..2^31, a non-null mask)", name);
        return false;
    }
    if (!mask_dtype_ok(mask_dtype)) {
        mi355_set_error("%s: unknown mask dtype %d (0 u8 / bool, 1 i32, 2 i64, 3 f32, 4 bf16)", name, mask_dtype);
        return false;
    }
    if (!dt_ok(x_dtype) || (mode != POOL_SCORES && !dt_ok(w_dtype))) {
        mi355_set_error("%s: hidden states and head are bf16 (0) or fp32 (1), got %d and %d", name, x_dtype, w_dtype);
        return false;
    }
    if (mode == POOL_SCORES) {
        if (E != 1) {
            mi355_set_error("%s: the scores of mode 0 are (B, S, 1), got a last dimension of %d", name, E);
            return false;
        }
        return true;
    }
    if (!(E >= 8 && E <= 8192 && E % 8 == 0)) {
        mi355_set_error("%s: emb_dim must be a multiple of 8 in 8..8192, got %d", name, E);
        return false;
    }
    if (!w || !aligned16(w)) {
        mi355_set_error("%s: the head's weight must be non-null and 16-byte aligned", name);
        return false;
    }
    return true;
}

extern "C" int mi355_reward_pool_fwd(int mode, int B, int64_t S, int E, const void* x, int x_dtype, const void* mask, int mask_dtype, const void* w,
                                     int w_dtype, const void* bias, float* score, float* pooled, float* count, void* stream) {
    if (!reward_pool_ok("mi355_reward_pool_fwd", mode, B, S, E, mask, mask_dtype, x_dtype, w, w_dtype)) return 1;
    MI355_REQUIRE(x && score && count, "mi355_reward_pool_fwd: bad arguments (null pointer)");
    if (mode == POOL_SCORES) {
        hipLaunchKernelGGL(reward_scores_fwd_kernel, dim3(B), dim3(256), 0, STREAM, S, x, x_dtype, mask, mask_dtype, score, count);
    } else {
        MI355_REQUIRE(pooled && aligned16(x) && aligned16(pooled), "mi355_reward_pool_fwd: the hidden states and the pooled rows must be non-null and 16-byte aligned");
        hipLaunchKernelGGL(reward_pool_fwd_kernel, dim3(B), dim3(256), 0, STREAM, mode, S, E, x, x_dtype, mask, mask_dtype, w, w_dtype, bias, score, pooled,
                           count);
    }
    MI355_LAUNCH_CHECK("mi355_reward_pool_fwd");
    return 0;
}

extern "C" int mi355_reward_pool_bwd(int mode, int B, int64_t S, int E, const float* g, const void* mask, int mask_dtype, const float* count,
                                     const void* w, int w_dtype, const float* pooled, void* dx, int x_dtype, void* dw, void* dbias, void* stream) {
    if (!reward_pool_ok("mi355_reward_pool_bwd", mode, B, S, E, mask, mask_dtype, x_dtype, w, w_dtype)) return 1;
    MI355_REQUIRE(g && count, "mi355_reward_pool_bwd: bad arguments (null pointer)");
    if (mode == POOL_SCORES) {
        MI355_REQUIRE(dx, "mi355_reward_pool_bwd: mode 0 has one gradient, the scores': dx must be non-null");
        hipLaunchKernelGGL(reward_scores_bwd_kernel, dim3(B), dim3(256), 0, STREAM, S, g, mask, mask_dtype, count, dx, x_dtype);
    } else {
        MI355_REQUIRE(dx || dw || dbias, "mi355_reward_pool_bwd: nothing to compute (dx, dw and dbias are all NULL)");
        MI355_REQUIRE(!dx || aligned16(dx), "mi355_reward_pool_bwd: dx must be 16-byte aligned");
        MI355_REQUIRE(!dw || pooled, "mi355_reward_pool_bwd: the weight gradient needs the pooled rows of the forward");
        if (dx) {
            const int64_t chunks = (int64_t)B * S * (E >> 3), blocks = (chunks + 255) / 256;
            hipLaunchKernelGGL(reward_pool_dx_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, STREAM, mode, chunks, S, E, g, mask,
                               mask_dtype, count, w, w_dtype, dx, x_dtype);
        }
        if (dw || dbias)
            hipLaunchKernelGGL(reward_pool_dw_kernel, dim3((E + 255) / 256), dim3(256), 0, STREAM, mode, B, E, g, count, pooled, dw, dbias, w_dtype);
    }
    MI355_LAUNCH_CHECK("mi355_reward_pool_bwd");
    return 0;
}
