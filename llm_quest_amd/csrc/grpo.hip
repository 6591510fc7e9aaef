// GRPO policy losses (alignment/rlhf_grpo/grpo_engine.py): the log-probability of each label over bf16 logits [B, S, V], its backward with one weight
// per token, the per-token loss chain of the five variants on fp32 [B, T] operands, and the one-pass form that reads a logits row once and overwrites
// it with d loss / d logits.  The row body restates the design of elementwise.hip's cross-entropy rows (that file is part of the step's source
// fingerprint and is not edited): 16-byte chunks, fp32 arithmetic, a fixed reduction order (per thread, per wave, the waves in order), 64-bit row
// addresses, and for the wide vocabularies the row held in registers between three opaque passes (maximum, sum, write).  No atomics anywhere.
#include <math.h>

#include "rows_bf16.h"

namespace {

enum { V_GRPO = 0, V_DAPO = 1, V_DR_GRPO = 2, V_SAPO = 3, V_GSPO = 4 };
enum { M_U8 = 0, M_I32 = 1, M_I64 = 2, M_F32 = 3, M_BF16 = 4 };

struct TokParams {
    float lo, hi, beta;  // 1 - min_clip, 1 + max_clip
    int variant, unbiased;
};

__device__ __forceinline__ float mask_at(const void* mask, int dt, int64_t i) {
    switch (dt) {
        case M_U8: return ((const uint8_t*)mask)[i] ? 1.f : 0.f;
        case M_I32: return (float)((const int32_t*)mask)[i];
        case M_I64: return (float)((const int64_t*)mask)[i];
        case M_F32: return ((const float*)mask)[i];
        default: return bf2f(((const bf16_t*)mask)[i]);
    }
}

// min(r A, clip(r, lo, hi) A) and its derivative in r as autograd takes it: torch.min of equal operands gives each half of the gradient, torch.clip
// passes it on the closed interval [lo, hi].
__device__ __forceinline__ void clipped_surrogate(float r, float A, float lo, float hi, float& s, float& ds) {
    const float u = r * A, c = fminf(fmaxf(r, lo), hi) * A;
    const float dc = (r >= lo && r <= hi) ? A : 0.f;
    if (u < c) s = u, ds = A;
    else if (u > c) s = c, ds = dc;
    else s = (u != u) ? u : c, ds = 0.5f * A + 0.5f * dc;  // equal (or unordered: NaN goes through like torch.min)
}

// One token of a token-level variant, before the mask and the normaliser: loss = -(surrogate * opm - beta * kl), dl = d loss / d policy_logp, kl = the
// k3 estimate exp(ref - pol) - (ref - pol) - 1, times the ratio when `unbiased` (the ratio is then differentiated too).  The off-policy mask opm and the
// SAPO temperature choice carry no gradient.
__device__ __forceinline__ void token_term(float pl, float ol, float rl, float A, float opm, const TokParams& P, float& loss, float& dl, float& kl) {
    const float r = expf(pl - ol);
    const float lr = rl - pl, q = expf(lr);
    const float k3 = q - lr - 1.f;
    float dkl = 1.f - q;
    kl = k3;
    if (P.unbiased) {
        kl = r * k3;
        dkl = r * k3 + r * (1.f - q);
    }
    float s, ds;
    if (P.variant == V_SAPO) {
        const float temp = A > 0.f ? 1.0f : 1.05f;
        const float sg = 1.f / (1.f + expf(-temp * (r - 1.f)));
        s = sg * 4.f / temp * A;
        ds = 4.f * A * sg * (1.f - sg);
    } else {
        clipped_surrogate(r, A, P.lo, P.hi, s, ds);
    }
    loss = -(s * opm - P.beta * kl);
    dl = -(ds * r * opm - P.beta * dkl);
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {  // fixed order: lanes by the xor tree, then the four waves
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// The loss sums are kept in fp64 (a few thousand additions per step): what the scalar loss then carries is the rounding of its fp32 terms alone.
__device__ __forceinline__ double block_sum_256(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// The factor that turns sequence b's masked token sum into its share of the scalar loss, in fp64 (the fp32 wn[b] of the gradients is its rounding).
__device__ __forceinline__ double seq_weight(int variant, int B, float cnt_b, float total, int max_gen) {
    if (variant == V_GRPO || variant == V_SAPO) return 1.0 / ((double)B * fmax((double)cnt_b, 1.0));
    if (variant == V_DAPO) return 1.0 / fmax((double)total, 1.0);
    if (variant == V_DR_GRPO) return 1.0 / ((double)B * (double)max_gen);
    return 1.0 / (double)B;
}

// ------------------------------------------------------------------------------------------- normalisers
// One workgroup.  cnt[b] = number of live tokens of sequence b (wave w takes sequences w, w + 16, ...; counts are exact in fp32 whatever the order),
// their total to cnt[B], then w[b], the factor that turns sequence b's masked token sum into its share of the scalar loss:
//   grpo / sapo 1 / (B max(1, cnt_b))  (equal groups: the mean over groups of the group means is the mean over B),  dapo 1 / max(1, total),
//   dr_grpo 1 / (B max_gen),  gspo 1 / B.
__global__ __launch_bounds__(1024) void grpo_seq_norm_kernel(int B, int64_t T, const void* __restrict__ mask, int mdt, int variant, int max_gen,
                                                             float* __restrict__ cnt, float* __restrict__ wn) {
    __shared__ float total;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int b = wid; b < B; b += 16) {
        float c = 0.f;
        for (int64_t t = lane; t < T; t += 64) c += mask_at(mask, mdt, (int64_t)b * T + t);
        c = wave_sum(c);
        if (lane == 0) cnt[b] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += cnt[b];
        total = s;
        cnt[B] = s;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 1024) wn[b] = (float)seq_weight(variant, B, cnt[b], total, max_gen);
}

// seq[b] = w_b sum_t terms[b, t] (thread i adds tokens i, i + 256, ... ascending, then the block tree)
__global__ __launch_bounds__(256) void grpo_seq_sum_kernel(int B, int64_t T, const float* __restrict__ terms, const float* __restrict__ cnt, int variant,
                                                           int max_gen, double* __restrict__ seq) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) s += (double)terms[(int64_t)b * T + t];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) seq[b] = s * seq_weight(variant, B, cnt[b], cnt[B], max_gen);
}

// loss[0] = sum_b seq[b], same order as above over the sequences, rounded to fp32 once
__global__ __launch_bounds__(256) void grpo_finish_kernel(int B, const double* __restrict__ seq, float* __restrict__ loss) {
    __shared__ double red[4];
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) s += seq[b];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) loss[0] = (float)s;
}

// ------------------------------------------------------------------------------------------- per-token chain
// One workgroup per sequence.  Pass A: the masked sums of the sequence (KL, policy and old log-probs), from which the mean KL, the off-policy mask
// and GSPO's sequence ratio follow.  Pass B: the per-token loss terms and d loss / d policy_logp, already weighted by w[b].
__global__ __launch_bounds__(256) void grpo_token_loss_kernel(int64_t T, const float* __restrict__ pol, const float* __restrict__ old,
                                                              const float* __restrict__ ref, const float* __restrict__ adv,
                                                              const void* __restrict__ mask, int mdt, TokParams P, float delta, int use_opm,
                                                              const float* __restrict__ cnt, const float* __restrict__ wn,
                                                              float* __restrict__ dlogp, uint8_t* __restrict__ opm_out,
                                                              float* __restrict__ mean_kl, double* __restrict__ seq, int max_gen) {
    __shared__ double redd[4];
    const int b = blockIdx.x, B = gridDim.x;
    const double wd = seq_weight(P.variant, B, cnt[b], cnt[B], max_gen);
    const int64_t o = (int64_t)b * T;
    const float A = adv[b], c = cnt[b], w = wn[b];
    TokParams Pk = P;
    if (P.variant == V_GSPO) Pk.unbiased = 0;  // the sequence-level ratio does not weigh a token's KL
    double skl = 0.0, spl = 0.0, sol = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) {
        const float m = mask_at(mask, mdt, o + t);
        float l, d, kl;
        token_term(pol[o + t], old[o + t], ref[o + t], A, 1.f, Pk, l, d, kl);
        skl += (double)(kl * m);
        spl += (double)(pol[o + t] * m);
        sol += (double)(old[o + t] * m);
    }
    skl = block_sum_256(skl, redd);
    const float mkl = (float)(skl / fmax((double)c, 1.0));
    const float opm = (!use_opm || A >= 0.f || mkl <= delta) ? 1.f : 0.f;
    if (threadIdx.x == 0) {
        mean_kl[b] = mkl;
        opm_out[b] = opm != 0.f;
    }
    if (P.variant == V_GSPO) {
        spl = block_sum_256(spl, redd);
        sol = block_sum_256(sol, redd);
        const float R = expf((float)(spl / (double)c) - (float)(sol / (double)c));  // an empty mask: 0 / 0, NaN, as log_probs_per_seq gives upstream
        float s, ds;
        clipped_surrogate(R, A, P.lo, P.hi, s, ds);
        if (threadIdx.x == 0) seq[b] = -(double)(s * opm) * wd;
        if (dlogp) {
            const float g = -(ds * opm) * R * w / c;
            for (int64_t t = threadIdx.x; t < T; t += 256) dlogp[o + t] = g * mask_at(mask, mdt, o + t);
        }
        return;
    }
    double sl = 0.0;
    for (int64_t t = threadIdx.x; t < T; t += 256) {
        const float m = mask_at(mask, mdt, o + t);
        float l, d, kl;
        token_term(pol[o + t], old[o + t], ref[o + t], A, opm, P, l, d, kl);
        sl += (double)(l * m);
        if (dlogp) dlogp[o + t] = d * m * w;
    }
    sl = block_sum_256(sl, redd);
    if (threadIdx.x == 0) seq[b] = sl * wd;
}

// ------------------------------------------------------------------------------------------- the pieces
// The reference-named per-token functions, one at a time (mi355_grpo_piece): one workgroup per sequence, thread i takes tokens i, i + 256, ...; x1 is a
// per-sequence vector [B] where an op takes advantages; wn the normalisers of grpo_seq_norm_kernel where an op aggregates.
enum {
    OP_KL_FWD = 1, OP_KL_BWD = 2, OP_SURR_FWD = 3, OP_SURR_BWD = 4, OP_SEQ_MEAN_FWD = 5, OP_SEQ_MEAN_BWD = 6, OP_RATIO_LOSS = 7, OP_GSPO_LOSS = 8,
    OP_AGGREGATE = 9, OP_OFF_POLICY = 10, OP_SCALE = 11
};
__device__ __forceinline__ void surrogate(float r, float A, float p0, float p1, int sapo, float& s, float& ds) {
    if (sapo) {  // p0, p1: the temperatures of tokens with a positive / another advantage
        const float temp = A > 0.f ? p0 : p1;
        const float sg = 1.f / (1.f + expf(-temp * (r - 1.f)));
        s = sg * 4.f / temp * A;
        ds = 4.f * A * sg * (1.f - sg);
    } else {
        clipped_surrogate(r, A, 1.f - p0, 1.f + p1, s, ds);
    }
}
__global__ __launch_bounds__(256) void grpo_piece_kernel(int op, int64_t T, const float* __restrict__ x0, const float* __restrict__ x1,
                                                         const float* __restrict__ x2, const float* __restrict__ x3, const void* __restrict__ mask,
                                                         int mdt, float p0, float p1, float p2, int flag, int variant, int max_gen,
                                                         const float* __restrict__ cnt, const float* __restrict__ wn, double* __restrict__ seq,
                                                         float* __restrict__ y0, float* __restrict__ y1, float* __restrict__ y2) {
    __shared__ float red[4];
    __shared__ double redd[4];
    const int b = blockIdx.x, B = gridDim.x;
    const int64_t o = (int64_t)b * T;
    switch (op) {
        case OP_KL_FWD:  // x0 pol, x1 ref, x2 ratio or NULL -> y0 = [ratio] (exp(ref - pol) - (ref - pol) - 1)
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                const float lr = x1[o + t] - x0[o + t], k3 = expf(lr) - lr - 1.f;
                y0[o + t] = x2 ? x2[o + t] * k3 : k3;
            }
            break;
        case OP_KL_BWD:  // + x3 = d/d kl -> y0 d/d pol, y1 d/d ref, y2 d/d ratio (with x2)
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                const float lr = x1[o + t] - x0[o + t], q = expf(lr), g = x3[o + t], rho = x2 ? x2[o + t] : 1.f;
                y0[o + t] = g * rho * (1.f - q);
                y1[o + t] = g * rho * (q - 1.f);
                if (x2) y2[o + t] = g * (q - lr - 1.f);
            }
            break;
        case OP_SURR_FWD:  // x0 ratio, x1 advantages [B] -> y0; flag: sapo
        case OP_SURR_BWD:  // + x3 = d/d surrogate -> y0 = d/d ratio
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                float s, ds;
                surrogate(x0[o + t], x1[b], p0, p1, flag, s, ds);
                y0[o + t] = op == OP_SURR_FWD ? s : x3[o + t] * ds;
            }
            break;
        case OP_SEQ_MEAN_FWD:    // x0 log-probs -> y0[b] = sum(x0 mask) / sum(mask)   (an empty mask: NaN, as upstream)
        case OP_SEQ_MEAN_BWD: {  // x3[b] = d/d mean -> y0[b, t] = x3[b] mask / sum(mask)
            float c = 0.f;
            double s = 0.0;
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                const float m = mask_at(mask, mdt, o + t);
                c += m;
                if (op == OP_SEQ_MEAN_FWD) s += (double)(x0[o + t] * m);
            }
            c = block_sum_256(c, red);
            if (op == OP_SEQ_MEAN_FWD) {
                s = block_sum_256(s, redd);
                if (threadIdx.x == 0) y0[b] = (float)(s / (double)c);
            } else {
                for (int64_t t = threadIdx.x; t < T; t += 256) y0[o + t] = x3[b] * mask_at(mask, mdt, o + t) / c;
            }
            break;
        }
        case OP_RATIO_LOSS: {  // GRPOLoss.compute, token level: x0 ratio, x1 advantages, x2 kl, x3 off-policy mask [B] as 0 / 1 or NULL; p2 beta
            double sl = 0.0;    // -> seq[b] = the sequence's share of the loss, y1 = d/d ratio, y2 = d/d kl
            const float opm = x3 ? x3[b] : 1.f, w = wn[b];
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                const float m = mask_at(mask, mdt, o + t);
                float s, ds;
                surrogate(x0[o + t], x1[b], flag ? 1.0f : p0, flag ? 1.05f : p1, flag, s, ds);  // sapo: the reference's default temperatures
                sl += (double)(-(s * opm - p2 * x2[o + t]) * m);
                y1[o + t] = -(ds * opm) * m * w;
                y2[o + t] = p2 * m * w;
            }
            sl = block_sum_256(sl, redd);
            if (threadIdx.x == 0) seq[b] = sl * seq_weight(variant, B, cnt[b], cnt[B], max_gen);
            break;
        }
        case OP_GSPO_LOSS: {  // one workgroup, T = the batch: x0 ratio [B], x1 advantages [B], x3 mask [B] or NULL -> y0[0] = mean(-surrogate), y1 = d/d ratio
            double sl = 0.0;
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                float s, ds;
                const float opm = x3 ? x3[t] : 1.f;
                clipped_surrogate(x0[t], x1[t], 1.f - p0, 1.f + p1, s, ds);
                sl += -(double)(s * opm);
                y1[t] = -(ds * opm) / (float)T;
            }
            sl = block_sum_256(sl, redd);
            if (threadIdx.x == 0) y0[0] = (float)(sl / (double)T);
            break;
        }
        case OP_AGGREGATE: {  // GRPOLoss._aggregate: x0 the (already masked) loss per token -> seq[b] = w[b] sum_t x0, y1[b, t] = w[b]
            double sl = 0.0;
            const float w = wn[b];
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                sl += (double)x0[o + t];
                y1[o + t] = w;
            }
            sl = block_sum_256(sl, redd);
            if (threadIdx.x == 0) seq[b] = sl * seq_weight(variant, B, cnt[b], cnt[B], max_gen);
            break;
        }
        case OP_OFF_POLICY: {  // x0 kl, x1 advantages, p0 delta -> y0[b] = masked mean kl, y1[b] = (A >= 0) | (mean <= delta) as 0 / 1
            float c = 0.f;
            double s = 0.0;
            for (int64_t t = threadIdx.x; t < T; t += 256) {
                const float m = mask_at(mask, mdt, o + t);
                c += m;
                s += (double)(x0[o + t] * m);
            }
            c = block_sum_256(c, red);
            s = block_sum_256(s, redd);
            const float mkl = (float)(s / fmax((double)c, 1.0));
            if (threadIdx.x == 0) {
                y0[b] = mkl;
                y1[b] = (x1[b] >= 0.f || mkl <= p0) ? 1.f : 0.f;
            }
            break;
        }
        default:  // OP_SCALE: y0 = x0 * x3[0]
            for (int64_t t = threadIdx.x; t < T; t += 256) y0[o + t] = x0[o + t] * x3[0];
    }
}

// ------------------------------------------------------------------------------------------- logits rows
// log-sum-exp of one row by a 256-thread block: online maximum / sum over 16-byte chunks, a scalar tail for V % 8, then the waves in order.  -inf
// entries are legal; a thread or wave that saw none but -inf carries (-inf, 0).
__device__ __forceinline__ float row_lse_256(const bf16_t* __restrict__ lr, int64_t V, float* red_m, float* red_s) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float m = -INFINITY, s = 0.f;
    const int64_t nv = V >> 3;
    for (int64_t i = threadIdx.x; i < nv; i += 256) {
        float v[8];
        unpack8(*reinterpret_cast<const u32x4*>(lr + i * 8), v);
        float vm = v[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) vm = fmaxf(vm, v[e]);
        if (vm > m) {
            s *= __expf(m - vm);
            m = vm;
        }
        if (m != -INFINITY) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += __expf(v[e] - m);
        }
    }
    for (int64_t i = (nv << 3) + threadIdx.x; i < V; i += 256) {
        const float v = bf2f(lr[i]);
        if (v > m) {
            s *= __expf(m - v);
            m = v;
        }
        if (m != -INFINITY) s += __expf(v - m);
    }
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
    __syncthreads();  // protects red_* reuse across rows
    if (lane == 0) {
        red_m[wid] = wm;
        red_s[wid] = s;
    }
    __syncthreads();
    const float bm = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float bs = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) bs += red_m[wv] == -INFINITY ? 0.f : red_s[wv] * __expf(red_m[wv] - bm);
    return bm + logf(bs);  // once per row: the accurate logarithm
}

// row[i] = bf16(g * (onehot(tgt)[i] - exp(row[i] - lse))); src == dst is allowed (each element is read, then written, by one thread)
__device__ __forceinline__ void write_grad_row_256(const bf16_t* lr, bf16_t* dr, int64_t V, int64_t tgt, float lse, float g) {
    const int64_t nv = V >> 3;
    for (int64_t i = threadIdx.x; i < nv; i += 256) {
        float v[8], o[8];
        unpack8(*reinterpret_cast<const u32x4*>(lr + i * 8), v);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = g * (((i * 8 + e) == tgt ? 1.0f : 0.0f) - __expf(v[e] - lse));
        *reinterpret_cast<u32x4*>(dr + i * 8) = pack8(o);
    }
    for (int64_t i = (nv << 3) + threadIdx.x; i < V; i += 256) dr[i] = f2bf(g * ((i == tgt ? 1.0f : 0.0f) - __expf(bf2f(lr[i]) - lse)));
}
__device__ __forceinline__ void zero_row_256(bf16_t* dr, int64_t V) {
    const int64_t nv = V >> 3;
    for (int64_t i = threadIdx.x; i < nv; i += 256) *reinterpret_cast<u32x4*>(dr + i * 8) = (u32x4){0, 0, 0, 0};
    for (int64_t i = (nv << 3) + threadIdx.x; i < V; i += 256) dr[i] = 0;
}

// logp[b, s] = logits[b, s, ids[b, s + 1]] - lse[b, s] for s < S - 1: the shift is in the addressing.  A label outside [0, V): NaN for that token.
__global__ __launch_bounds__(256) void label_logprob_fwd_kernel(int64_t rows, int64_t S, int64_t V, const bf16_t* __restrict__ logits, int64_t bstride,
                                                                int64_t ldl, const int64_t* __restrict__ ids, float* __restrict__ logp,
                                                                float* __restrict__ lse_out) {
    __shared__ float red_m[4], red_s[4];
    const int64_t T = S - 1;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / T, s = row - b * T;
        const bf16_t* lr = logits + b * bstride + s * ldl;
        const int64_t tgt = ids[b * S + s + 1];
        const float lse = row_lse_256(lr, V, red_m, red_s);
        if (threadIdx.x == 0) {
            lse_out[row] = lse;
            logp[row] = (tgt < 0 || tgt >= V) ? __builtin_nanf("") : bf2f(lr[tgt]) - lse;
        }
    }
}

// dlogits[b, s, :] = g[b, s] (onehot - exp(logits - lse)) for s < S - 1, exact zeros for s = S - 1 (and for a label outside [0, V), as the CE rows do)
__global__ __launch_bounds__(256) void label_logprob_bwd_kernel(int64_t rows, int64_t S, int64_t V, const float* __restrict__ g,
                                                                const bf16_t* logits, int64_t bstride, int64_t ldl, const float* __restrict__ lse,
                                                                const int64_t* __restrict__ ids, bf16_t* dlogits, int64_t dbstride, int64_t ldd) {
    const int64_t T = S - 1;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / S, s = row - b * S;
        const bf16_t* lr = logits + b * bstride + s * ldl;
        bf16_t* dr = dlogits + b * dbstride + s * ldd;
        const int64_t tgt = s < T ? ids[b * S + s + 1] : -1;
        if (tgt < 0 || tgt >= V) {
            zero_row_256(dr, V);
            continue;
        }
        write_grad_row_256(lr, dr, V, tgt, lse[b * T + s], g[b * T + s]);
    }
}

// What thread 0 of a one-pass row does once the row's lse is known: the token's log-prob, loss term and the weight of the row's gradient.
struct RowOperands {
    const int64_t* ids;
    const float *old, *ref, *adv, *wn;
    const void* mask;
    int mdt;
    float *terms, *logp, *lse;
};
__device__ __forceinline__ float row_token(const RowOperands& R, const TokParams& P, int64_t b, int64_t s, int64_t T, float tgt_logit, float lse) {
    const int64_t t = b * T + s;
    const float pl = tgt_logit - lse, m = mask_at(R.mask, R.mdt, t), w = R.wn[b];
    float l, d, kl;
    token_term(pl, R.old[t], R.ref[t], R.adv[b], 1.f, P, l, d, kl);
    if (threadIdx.x == 0) {
        R.logp[t] = pl;
        R.terms[t] = l * m;
    }
    return d * m * w;
}

// The one-pass path, any V: the row is read for its lse, then re-read (from L2 / Infinity Cache) and overwritten with its gradient.
__global__ __launch_bounds__(256) void grpo_logits_rows_kernel(int64_t rows, int64_t S, int64_t V, const bf16_t* logits, int64_t bstride, int64_t ldl,
                                                               bf16_t* dlogits, int64_t dbstride, int64_t ldd, RowOperands R, TokParams P) {
    __shared__ float red_m[4], red_s[4];
    const int64_t T = S - 1;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / S, s = row - b * S;
        const bf16_t* lr = logits + b * bstride + s * ldl;
        bf16_t* dr = dlogits + b * dbstride + s * ldd;
        if (s == T) {
            zero_row_256(dr, V);
            continue;
        }
        const int64_t tgt = R.ids[b * S + s + 1];
        const bool ok = tgt >= 0 && tgt < V;
        // read before the barriers: in place the other waves overwrite the row behind them
        const float tgt_logit = ok ? bf2f(lr[tgt]) : __builtin_nanf("");
        const float lse = row_lse_256(lr, V, red_m, red_s);
        const float g = row_token(R, P, b, s, T, tgt_logit, lse);
        if (!ok) zero_row_256(dr, V);
        else write_grad_row_256(lr, dr, V, tgt, lse, g);
    }
}

// The same with the row kept in registers: one 1024-thread block per row, thread t holds the 16-byte chunks t, t + 1024, ... (NCH of them: 76
// registers at NCH = 19, a vocabulary up to 155 648), so the logits are read from memory ONCE.  Needs V % 8 == 0.  Every index into the chunk array is
// a compile-time constant (dynamic indexing would put the array in scratch); the asm statements keep one pass's unpacked values from being kept for
// the next (152 floats per thread: they would spill), the scheduling barriers keep the chunks one at a time.
// FWD: the label log-prob forward alone (logp and lse, nothing written to the row) with the very same reduction, so that the two paths' log-probs are the same bits.
template <int NCH, bool FWD>
__global__ __launch_bounds__(1024) void grpo_logits_regs_kernel(int64_t rows, int64_t S, int64_t V, const bf16_t* logits, int64_t bstride, int64_t ldl,
                                                                bf16_t* dlogits, int64_t dbstride, int64_t ldd, RowOperands R, TokParams P) {
    __shared__ float red_m[16], red_s[16];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nv = (int)(V >> 3);
    const unsigned tid8 = threadIdx.x * 8;
    const int64_t T = S - 1;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / S, s = row - b * S;
        const bf16_t* lr = logits + b * bstride + s * ldl;
        bf16_t* dr = FWD ? nullptr : dlogits + b * dbstride + s * ldd;
        const int64_t tgt = s < T ? R.ids[b * S + s + 1] : -1;
        const bool ok = tgt >= 0 && tgt < V;
        if (s == T) {
            if (!FWD)
                for (int i = threadIdx.x; i < nv; i += 1024) *reinterpret_cast<u32x4*>(dr + (int64_t)i * 8) = (u32x4){0, 0, 0, 0};
            continue;
        }
        const float tgt_logit = ok ? bf2f(lr[tgt]) : __builtin_nanf("");  // before the barriers: in place, the row is overwritten behind them
        u32x4 r[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int i = threadIdx.x + 1024 * j;
            r[j] = i < nv ? *reinterpret_cast<const u32x4*>(lr + (int64_t)j * 8192 + tid8) : (u32x4){0xff80ff80u, 0xff80ff80u, 0xff80ff80u, 0xff80ff80u};  // -inf pairs
        }
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            float v[8];
            asm volatile("" : "+v"(r[j]));
            unpack8(r[j], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) m = fmaxf(m, v[e]);
            __builtin_amdgcn_sched_barrier(0);
        }
        m = wave_max(m);
        __syncthreads();  // protects red_* reuse across rows
        if (lane == 0) red_m[wid] = m;
        __syncthreads();
        float bm = red_m[0];
#pragma unroll
        for (int wv = 1; wv < 16; ++wv) bm = fmaxf(bm, red_m[wv]);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            float v[8];
            asm volatile("" : "+v"(r[j]));
            unpack8(r[j], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += __expf(v[e] - bm);  // exp(-inf) = 0 for the padding of the last chunks
            __builtin_amdgcn_sched_barrier(0);
        }
        sum = wave_sum(sum);
        if (lane == 0) red_s[wid] = sum;
        __syncthreads();
        float bs = 0.f;
#pragma unroll
        for (int wv = 0; wv < 16; ++wv) bs += red_s[wv];
        const float lse = bm + logf(bs);
        if (FWD) {
            if (threadIdx.x == 0) {
                R.lse[b * T + s] = lse;
                R.logp[b * T + s] = tgt_logit - lse;  // NaN for a label outside [0, V)
            }
            continue;
        }
        const float g = ok ? row_token(R, P, b, s, T, tgt_logit, lse) : (row_token(R, P, b, s, T, tgt_logit, lse), 0.f);
        const int tch = ok ? (int)(tgt >> 3) : -1, te = (int)(tgt & 7);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int i = threadIdx.x + 1024 * j;
            float v[8], o[8];
            asm volatile("" : "+v"(r[j]));
            unpack8(r[j], v);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = g * (((i == tch && e == te) ? 1.0f : 0.0f) - __expf(v[e] - lse));
            if (i < nv) *reinterpret_cast<u32x4*>(dr + (int64_t)j * 8192 + tid8) = pack8(o);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

bool grpo_logits_ok(const char* name, int64_t B, int64_t S, int64_t V, const void* logits, int64_t bstride, int64_t ldl) {
    if (!(B > 0 && B <= (1 << 24) && S >= 2 && S <= (1 << 24) && V > 0 && V <= (int64_t)1 << 31 && logits)) {
        mi355_set_error("%s: bad arguments (B in 1..2^24, S in 2..2^24, V in 1..2^31, non-null pointers)", name);
        return false;
    }
    if (!(ldl >= V && bstride >= 0 && (ldl & 7) == 0 && (bstride & 7) == 0 && ((uintptr_t)logits & 15) == 0)) {
        mi355_set_error("%s: the vector path needs 16-byte rows: pointer 16-byte aligned, row pitch >= V and batch stride multiples of 8 elements", name);
        return false;
    }
    return true;
}
bool grpo_scalars_ok(const char* name, float min_clip, float max_clip, float beta, int num_samples, int max_gen, int variant, int B, int mask_dtype) {
    if (!(variant >= V_GRPO && variant <= V_GSPO)) {
        mi355_set_error("%s: unknown variant %d (0 grpo, 1 dapo, 2 dr_grpo, 3 sapo, 4 gspo)", name, variant);
        return false;
    }
    if (!(mask_dtype >= M_U8 && mask_dtype <= M_BF16)) {
        mi355_set_error("%s: unknown mask dtype %d (0 u8 / bool, 1 i32, 2 i64, 3 f32, 4 bf16)", name, mask_dtype);
        return false;
    }
    if (!(min_clip == min_clip && max_clip == max_clip && beta == beta && num_samples > 0 && max_gen > 0)) {
        mi355_set_error("%s: clip bounds and beta must be numbers, num_samples and max_gen positive", name);
        return false;
    }
    if ((variant == V_GRPO || variant == V_SAPO) && B % num_samples != 0) {
        mi355_set_error("%s: the batch (%d) must be a multiple of num_samples (%d) for grpo / sapo", name, B, num_samples);
        return false;
    }
    return true;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int mi355_label_logprob_fwd(int64_t B, int64_t S, int64_t V, const void* logits, int64_t bstride, int64_t ldl, const int64_t* ids,
                                       float* logp, float* lse, void* stream) {
    if (!grpo_logits_ok("mi355_label_logprob_fwd", B, S, V, logits, bstride, ldl)) return 1;
    MI355_REQUIRE(ids && logp && lse, "mi355_label_logprob_fwd: bad arguments (null pointer)");
    const int64_t rows = B * (S - 1), all_rows = B * S, chunks = V >> 3;
    const RowOperands R = {ids, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, logp, lse};
    const TokParams P = {0.f, 0.f, 0.f, 0, 0};
    const unsigned grid = (unsigned)(all_rows < 65535 ? all_rows : 65535);
    const bf16_t* lg = (const bf16_t*)logits;
    // the widths of mi355_grpo_logits_loss, each with its reduction: the log-probs of the two paths are the same bits
    if ((V & 7) == 0 && chunks > 4 * 1024 && chunks <= 19 * 1024)
        hipLaunchKernelGGL((grpo_logits_regs_kernel<19, true>), dim3(grid), dim3(1024), 0, STREAM, all_rows, S, V, lg, bstride, ldl, (bf16_t*)nullptr, 0, 0, R, P);
    else if ((V & 7) == 0 && chunks > 1024 && chunks <= 4 * 1024)
        hipLaunchKernelGGL((grpo_logits_regs_kernel<4, true>), dim3(grid), dim3(1024), 0, STREAM, all_rows, S, V, lg, bstride, ldl, (bf16_t*)nullptr, 0, 0, R, P);
    else
        hipLaunchKernelGGL(label_logprob_fwd_kernel, dim3((unsigned)(rows < 65535 ? rows : 65535)), dim3(256), 0, STREAM, rows, S, V, lg, bstride, ldl, ids, logp, lse);
    MI355_LAUNCH_CHECK("mi355_label_logprob_fwd");
    return 0;
}

extern "C" int mi355_label_logprob_bwd(int64_t B, int64_t S, int64_t V, const float* g, const void* logits, int64_t bstride, int64_t ldl,
                                       const float* lse, const int64_t* ids, void* dlogits, int64_t dbstride, int64_t ldd, void* stream) {
    if (!grpo_logits_ok("mi355_label_logprob_bwd", B, S, V, logits, bstride, ldl)) return 1;
    if (!grpo_logits_ok("mi355_label_logprob_bwd", B, S, V, dlogits, dbstride, ldd)) return 1;
    MI355_REQUIRE(g && lse && ids, "mi355_label_logprob_bwd: bad arguments (null pointer)");
    MI355_REQUIRE(dlogits != logits || (dbstride == bstride && ldd == ldl), "mi355_label_logprob_bwd: in place needs the logits' own strides");
    const int64_t rows = B * S;
    hipLaunchKernelGGL(label_logprob_bwd_kernel, dim3((unsigned)(rows < 65535 ? rows : 65535)), dim3(256), 0, STREAM, rows, S, V, g,
                       (const bf16_t*)logits, bstride, ldl, lse, ids, (bf16_t*)dlogits, dbstride, ldd);
    MI355_LAUNCH_CHECK("mi355_label_logprob_bwd");
    return 0;
}

extern "C" int mi355_grpo_token_loss(int B, int64_t T, const float* policy_logp, const float* old_logp, const float* ref_logp, const float* advantages,
                                     const void* loss_mask, int mask_dtype, float min_clip, float max_clip, float beta, float delta, int num_samples,
                                     int max_gen, int variant, int unbiased_kl, int use_off_policy_mask, float* loss, float* dlogp,
                                     uint8_t* off_policy_mask, float* mean_kl, float* workspace, void* stream) {
    MI355_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= ((int64_t)1 << 31) && policy_logp && old_logp && ref_logp && advantages && loss_mask && loss &&
                      off_policy_mask && mean_kl && workspace,
                  "mi355_grpo_token_loss: bad arguments (B in 1..65535, T in 1..2^31, non-null pointers; dlogp alone may be NULL)");
    if (!grpo_scalars_ok("mi355_grpo_token_loss", min_clip, max_clip, beta, num_samples, max_gen, variant, B, mask_dtype)) return 1;
    MI355_REQUIRE(!use_off_policy_mask || delta == delta, "mi355_grpo_token_loss: the off-policy mask needs a number for delta");
    MI355_REQUIRE(((uintptr_t)workspace & 7) == 0, "mi355_grpo_token_loss: the workspace must be 8-byte aligned");
    double* seq = (double*)workspace;  // workspace: B fp64 sequence shares, B + 1 fp32 counts (and their total), B fp32 normalisers
    float *cnt = workspace + 2 * (int64_t)B, *wn = cnt + B + 1;
    const TokParams P = {1.f - min_clip, 1.f + max_clip, beta, variant, unbiased_kl != 0};
    hipLaunchKernelGGL(grpo_seq_norm_kernel, dim3(1), dim3(1024), 0, STREAM, B, T, loss_mask, mask_dtype, variant, max_gen, cnt, wn);
    hipLaunchKernelGGL(grpo_token_loss_kernel, dim3(B), dim3(256), 0, STREAM, T, policy_logp, old_logp, ref_logp, advantages, loss_mask, mask_dtype, P,
                       delta, use_off_policy_mask != 0, cnt, wn, dlogp, off_policy_mask, mean_kl, seq, max_gen);
    hipLaunchKernelGGL(grpo_finish_kernel, dim3(1), dim3(256), 0, STREAM, B, seq, loss);
    MI355_LAUNCH_CHECK("mi355_grpo_token_loss");
    return 0;
}

extern "C" int mi355_grpo_piece(int op, int B, int64_t T, const float* x0, const float* x1, const float* x2, const float* x3, const void* loss_mask,
                                int mask_dtype, float p0, float p1, float p2, int flag, int num_samples, int max_gen, float* y0, float* y1, float* y2,
                                float* workspace, void* stream) {
    MI355_REQUIRE(op >= OP_KL_FWD && op <= OP_SCALE, "mi355_grpo_piece: unknown op %d", op);
    MI355_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= ((int64_t)1 << 31) && x0 && y0, "mi355_grpo_piece: bad arguments (B in 1..65535, T in 1..2^31, x0 and y0 non-null)");
    const bool needs_mask = op == OP_SEQ_MEAN_FWD || op == OP_SEQ_MEAN_BWD || op == OP_RATIO_LOSS || op == OP_AGGREGATE || op == OP_OFF_POLICY;
    const bool aggregates = op == OP_RATIO_LOSS || op == OP_AGGREGATE;
    MI355_REQUIRE(!needs_mask || (loss_mask && mask_dtype >= M_U8 && mask_dtype <= M_BF16), "mi355_grpo_piece: op %d needs a loss mask of a known dtype", op);
    bool ok = true;
    switch (op) {
        case OP_KL_FWD: ok = x1; break;
        case OP_KL_BWD: ok = x1 && x3 && y1 && (!x2 || y2); break;
        case OP_SURR_FWD: ok = x1; break;
        case OP_SURR_BWD: ok = x1 && x3; break;
        case OP_SEQ_MEAN_BWD: ok = x3; break;
        case OP_RATIO_LOSS: ok = x1 && x2 && y1 && y2 && workspace; break;
        case OP_GSPO_LOSS: ok = x1 && y1 && B == 1; break;
        case OP_AGGREGATE: ok = y1 && workspace; break;
        case OP_OFF_POLICY: ok = x1 && y1; break;
        case OP_SCALE: ok = x3; break;
        default: break;
    }
    MI355_REQUIRE(ok, "mi355_grpo_piece: op %d misses an operand", op);
    float *cnt = nullptr, *wn = nullptr;
    double* seq = (double*)workspace;
    if (aggregates) {
        MI355_REQUIRE(((uintptr_t)workspace & 7) == 0, "mi355_grpo_piece: the workspace must be 8-byte aligned");
        MI355_REQUIRE(flag >= V_GRPO && flag <= V_SAPO, "mi355_grpo_piece: op %d aggregates a token-level variant (0 grpo, 1 dapo, 2 dr_grpo, 3 sapo), got %d", op, flag);
        if (!grpo_scalars_ok("mi355_grpo_piece", p0, p1, p2, num_samples, max_gen, flag, B, mask_dtype)) return 1;
        cnt = workspace + 2 * (int64_t)B, wn = cnt + B + 1;
        hipLaunchKernelGGL(grpo_seq_norm_kernel, dim3(1), dim3(1024), 0, STREAM, B, T, loss_mask, mask_dtype, flag, max_gen, cnt, wn);
    }
    const int kflag = op == OP_RATIO_LOSS ? flag == V_SAPO : flag;
    hipLaunchKernelGGL(grpo_piece_kernel, dim3(B), dim3(256), 0, STREAM, op, T, x0, x1, x2, x3, loss_mask, mask_dtype, p0, p1, p2, kflag, flag, max_gen, cnt, wn,
                       seq, y0, y1, y2);
    if (aggregates) hipLaunchKernelGGL(grpo_finish_kernel, dim3(1), dim3(256), 0, STREAM, B, seq, y0);
    MI355_LAUNCH_CHECK("mi355_grpo_piece");
    return 0;
}

extern "C" int mi355_grpo_logits_loss(int B, int64_t S, int64_t V, const void* logits, int64_t bstride, int64_t ldl, void* dlogits, int64_t dbstride,
                                      int64_t ldd, const int64_t* ids, const float* old_logp, const float* ref_logp, const float* advantages,
                                      const void* loss_mask, int mask_dtype, float min_clip, float max_clip, float beta, int num_samples, int max_gen,
                                      int variant, int unbiased_kl, int use_off_policy_mask, float* loss, float* terms, float* policy_logp,
                                      float* workspace, void* stream) {
    MI355_REQUIRE(variant != V_GSPO, "mi355_grpo_logits_loss: gspo needs a per-sequence ratio before any row's weight is known: use the two-pass path");
    MI355_REQUIRE(!use_off_policy_mask, "mi355_grpo_logits_loss: the off-policy mask needs a per-sequence KL before any row's weight is known: use the two-pass path");
    if (!grpo_logits_ok("mi355_grpo_logits_loss", B, S, V, logits, bstride, ldl)) return 1;
    if (!grpo_logits_ok("mi355_grpo_logits_loss", B, S, V, dlogits, dbstride, ldd)) return 1;
    MI355_REQUIRE(B <= 65535 && ids && old_logp && ref_logp && advantages && loss_mask && loss && terms && policy_logp && workspace,
                  "mi355_grpo_logits_loss: bad arguments (B in 1..65535, non-null pointers)");
    MI355_REQUIRE(dlogits != logits || (dbstride == bstride && ldd == ldl), "mi355_grpo_logits_loss: in place needs the logits' own strides");
    if (!grpo_scalars_ok("mi355_grpo_logits_loss", min_clip, max_clip, beta, num_samples, max_gen, variant, B, mask_dtype)) return 1;
    const int64_t T = S - 1, rows = (int64_t)B * S, chunks = V >> 3;
    MI355_REQUIRE(((uintptr_t)workspace & 7) == 0, "mi355_grpo_logits_loss: the workspace must be 8-byte aligned");
    double* seq = (double*)workspace;
    float *cnt = workspace + 2 * (int64_t)B, *wn = cnt + B + 1;
    const TokParams P = {1.f - min_clip, 1.f + max_clip, beta, variant, unbiased_kl != 0};
    const RowOperands R = {ids, old_logp, ref_logp, advantages, wn, loss_mask, mask_dtype, terms, policy_logp, nullptr};
    const unsigned grid = (unsigned)(rows < 65535 ? rows : 65535);
    const bf16_t* lg = (const bf16_t*)logits;
    bf16_t* dl = (bf16_t*)dlogits;
    hipLaunchKernelGGL(grpo_seq_norm_kernel, dim3(1), dim3(1024), 0, STREAM, B, T, loss_mask, mask_dtype, variant, max_gen, cnt, wn);
    if ((V & 7) == 0 && chunks > 4 * 1024 && chunks <= 19 * 1024)  // wide vocabularies: the row stays in registers, one read
        hipLaunchKernelGGL((grpo_logits_regs_kernel<19, false>), dim3(grid), dim3(1024), 0, STREAM, rows, S, V, lg, bstride, ldl, dl, dbstride, ldd, R, P);
    else if ((V & 7) == 0 && chunks > 1024 && chunks <= 4 * 1024)
        hipLaunchKernelGGL((grpo_logits_regs_kernel<4, false>), dim3(grid), dim3(1024), 0, STREAM, rows, S, V, lg, bstride, ldl, dl, dbstride, ldd, R, P);
    else
        hipLaunchKernelGGL(grpo_logits_rows_kernel, dim3(grid), dim3(256), 0, STREAM, rows, S, V, lg, bstride, ldl, dl, dbstride, ldd, R, P);
    hipLaunchKernelGGL(grpo_seq_sum_kernel, dim3(B), dim3(256), 0, STREAM, B, T, terms, cnt, variant, max_gen, seq);
    hipLaunchKernelGGL(grpo_finish_kernel, dim3(1), dim3(256), 0, STREAM, B, seq, loss);
    MI355_LAUNCH_CHECK("mi355_grpo_logits_loss");
    return 0;
}
