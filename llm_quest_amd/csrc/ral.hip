// Reinforced Attention Learning (reference common/reinforced_attention_learning.py, arXiv 2602.04884): the advantage-weighted Jensen-Shannon
// divergence between the head-averaged attention distributions of the policy and of the old policy.
//
// The reference is fed the materialised (b, heads, s, s) softmax, which no attention kernel here writes.  Two ways in:
//   from q, k (ours): the softmax of every head is recomputed from the post-RoPE q, k on the 32-key tile layer (attn_tile32.h; S^T = K Q^T with
//     the query on the MFMA lane, as llama3.hip's max-logit kernel) and only the head mean leaves the chip: P [B, S, S] fp32.  The backward is the
//     generic attention backward with the dP tile LOADED (the gradient on the head mean) instead of computed from dO and V, and a sweep of its own
//     for delta, for which there is no dO . O shortcut.  Rounding points of attention_generic.hip: dS rounded to bf16 before it enters an MFMA, one
//     bf16 rounding of dq / dk.
//   from weights (the reference's own entry): head mean, diagonal mask, renormalise, clamp over all S columns of [B, H, S, S] fp32 / bf16.
// Both leave   a(i,j) = mean_h p_h(i,j), diagonal 0;   Z(i) = max(sum_j a(i,j), 1e-8);   P(i,j) = max(a(i,j) / Z(i), 1e-8)  for every j in [0, S)
// and share the renormalisation backward, the JSD rows and the reduction.  Everything is fp32 except the bf16 q, k, dq, dk; a row is one wave, sums
// run in a fixed order, no atomics: two runs give the same bits.  Nothing is read back to the host.
#include "host_checks.h"

#include "attn_tile32.h"

namespace {

constexpr float RAL_EPS = 1e-8f;

// ------------------------------------------------------------------------------------------------ prepare from q, k: forward
// visible(query, key): key <= query and the key is a real token.  km = the sample's key-mask row or nullptr.
__device__ __forceinline__ bool ral_visible(bool qvalid, int query, int key, const uint8_t* __restrict__ km) {
    return qvalid && key <= query && (km == nullptr || km[key] != 0);
}

// grid (ceil(S / 128), B): a workgroup owns 128 queries of one sample and walks every head.  Sweep 1, per head: online max and sum over the key tiles
// up to the diagonal, with a second sum that leaves the diagonal out -- Z = mean_h l_excl_h / l_h has no 1 - p(i,i) cancellation.  Sweep 2, per key
// tile: sum_h exp2(s_h - lse_h) over the head loop (a K image is loaded once per kv head), then scale, clamp and store; the tiles above the
// workgroup's diagonal are stored as 1e-8 without a product.
template <int D>
__global__ __launch_bounds__(256) void ral_qk_fwd_kernel(int S, int Hq, int Hkv, const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                         int64_t ldk, const uint8_t* __restrict__ key_mask, float scale_log2, float* __restrict__ P,
                                                         float* __restrict__ Z, float* __restrict__ lse) {
    using C = Tile32<D>;
    __shared__ __attribute__((aligned(16))) char kimg[C::IMG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, rep = Hq / Hkv;
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    const int ndiag = qlast / 32 + 1;  // key tiles that hold a pair at or below the workgroup's diagonal
    const uint8_t* km = key_mask ? key_mask + tok0 : nullptr;
    const bf16_t* qrow = q + (tok0 + (qvalid ? query : 0)) * ldq;
    bf16x8 qf[C::KS];
    float zsum = 0.f;
    for (int h = 0; h < Hq; ++h) {
        const int hkv = h / rep;
        load_row_frags<D>(qrow + (int64_t)h * D, qvalid, lane, qf);
        float m = NEG_INF, l = 0.f, lx = 0.f;
        for (int kt = 0; kt < ndiag; ++kt) {
            const int key0 = kt * 32;
            __syncthreads();
            load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
            __syncthreads();
            if (q0 >= S || key0 > q0 + 31) continue;  // above this wave's diagonal
            f32x16 s;
            zero_tile(s);
            mma_rows<D>(s, kimg, qf, lane);
            float mx = NEG_INF;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = key0 + acc_row(i, lane);
                s[i] = ral_visible(qvalid, query, key, km) ? s[i] * scale_log2 : NEG_INF;
                mx = fmaxf(mx, s[i]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m, mx);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;
            const float alpha = exp2f(m - m_use);
            float rs = 0.f, rx = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = exp2f(s[i] - m_use);
                rs += p;
                rx += key0 + acc_row(i, lane) == query ? 0.f : p;
            }
            rs += __shfl_xor(rs, 32, 64);
            rx += __shfl_xor(rx, 32, 64);
            l = l * alpha + rs;
            lx = lx * alpha + rx;
            m = m_new;
        }
        if (l > 0.f) zsum += lx / l;
        if (lane < 32 && qvalid) lse[((int64_t)b * Hq + h) * S + query] = (m + log2f(l)) * LN2;  // -inf for a row without a visible key
    }
    __syncthreads();  // the lse rows of this workgroup, written by its own lanes, are read back below
    const float zc = fmaxf(zsum / (float)Hq, RAL_EPS);
    if (lane < 32 && qvalid) Z[tok0 + query] = zc;
    const int ntiles = (S + 31) / 32;
    for (int kt = 0; kt < ntiles; ++kt) {
        const int key0 = kt * 32;
        f32x16 acc;
        zero_tile(acc);
        if (kt < ndiag) {
            for (int h = 0; h < Hq; ++h) {
                const int hkv = h / rep;
                if (h % rep == 0) {
                    __syncthreads();
                    load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
                    __syncthreads();
                }
                if (q0 >= S || key0 > q0 + 31) continue;
                load_row_frags<D>(qrow + (int64_t)h * D, qvalid, lane, qf);
                const float lse2 = qvalid ? lse[((int64_t)b * Hq + h) * S + query] * LOG2E : 0.f;
                f32x16 s;
                zero_tile(s);
                mma_rows<D>(s, kimg, qf, lane);
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = key0 + acc_row(i, lane);
                    acc[i] += ral_visible(qvalid, query, key, km) ? exp2f(s[i] * scale_log2 - lse2) : 0.f;
                }
            }
        }
        float* prow = P + (tok0 + (qvalid ? query : 0)) * S;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const float a = (key == query ? 0.f : acc[i]) / (float)Hq;
            if (qvalid && key < S) prow[key] = fmaxf(a / zc, RAL_EPS);
        }
    }
}

// ------------------------------------------------------------------------------------------------ prepare from q, k: backward
// the gradient on a(query, key): read strictly below the diagonal only (the diagonal of a is a constant 0)
__device__ __forceinline__ float ral_da(const float* __restrict__ darow, bool ok, int query, int key) { return (ok && key < query) ? darow[key] : 0.f; }

// query-major pass, grid (ceil(S / 128), Hq, B).  Sweep 1: delta_h(i) = (1 / Hq) sum_j p_h(i,j) da(i,j), stored for the key-major pass.
// Sweep 2: dS = p (da / Hq - delta) scale, rounded to bf16, dQ^T += K^T dS^T.
template <int D>
__global__ __launch_bounds__(256) void ral_qk_bwd_dq_kernel(int S, int Hq, int Hkv, const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                            int64_t ldk, const uint8_t* __restrict__ key_mask, float scale, const float* __restrict__ da,
                                                            const float* __restrict__ lse, float* __restrict__ delta, bf16_t* __restrict__ dq,
                                                            int64_t lddq) {
    using C = Tile32<D>;
    __shared__ __attribute__((aligned(16))) char kimg[C::IMG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hkv = h / (Hq / Hkv);
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    const int ndiag = qlast / 32 + 1;
    const uint8_t* km = key_mask ? key_mask + tok0 : nullptr;
    const float* darow = da + (tok0 + (qvalid ? query : 0)) * S;
    bf16x8 qf[C::KS];
    load_row_frags<D>(q + (tok0 + (qvalid ? query : 0)) * ldq + (int64_t)h * D, qvalid, lane, qf);
    const float lse2 = qvalid ? lse[((int64_t)b * Hq + h) * S + query] * LOG2E : 0.f;
    const float scale_log2 = scale * LOG2E, inv_h = 1.f / (float)Hq;
    float dl = 0.f;
    for (int kt = 0; kt < ndiag; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31) continue;
        f32x16 s;
        zero_tile(s);
        mma_rows<D>(s, kimg, qf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = ral_visible(qvalid, query, key, km);
            const float p = ok ? exp2f(s[i] * scale_log2 - lse2) : 0.f;
            dl += p * ral_da(darow, ok, query, key);
        }
    }
    dl += __shfl_xor(dl, 32, 64);
    dl *= inv_h;
    if (lane < 32 && qvalid) delta[((int64_t)b * Hq + h) * S + query] = dl;
    f32x16 acc[C::DT];
    zero_tiles(acc);
    for (int kt = 0; kt < ndiag; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31) continue;
        f32x16 s;
        zero_tile(s);
        mma_rows<D>(s, kimg, qf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = ral_visible(qvalid, query, key, km);
            const float p = ok ? exp2f(s[i] * scale_log2 - lse2) : 0.f;
            s[i] = p * (ral_da(darow, ok, query, key) * inv_h - dl) * scale;
        }
        const bf16x8 d0 = pack_frag(s, 0), d1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) mma_cols<D>(acc[dt], kimg, 32 * dt, d0, d1, lane);
    }
    store_t_tiles<C::DT>(acc, 1.f, dq + (tok0 + query) * lddq + (int64_t)h * D, qvalid, lane);
}

// key-major pass, grid (ceil(S / 128), Hkv, B): a wave owns 32 keys of one kv head and walks the query heads of its group and the query tiles from
// the diagonal on (attention_generic.hip's dK/dV pass without the V half).  dK^T += Q^T dS.
template <int D>
__global__ __launch_bounds__(256) void ral_qk_bwd_dk_kernel(int S, int Hq, int Hkv, const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                            int64_t ldk, const uint8_t* __restrict__ key_mask, float scale, const float* __restrict__ da,
                                                            const float* __restrict__ lse, const float* __restrict__ delta, bf16_t* __restrict__ dk,
                                                            int64_t lddk) {
    using C = Tile32<D>;
    __shared__ __attribute__((aligned(16))) char qimg[C::IMG];
    __shared__ float stat[2][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, hkv = blockIdx.y, rep = Hq / Hkv;
    const int kb = blockIdx.x;
    const int k0 = kb * 128 + wave * 32;
    const int key = k0 + (lane & 31);
    const bool kvalid = key < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 kf[C::KS];
    load_row_frags<D>(k + (tok0 + (kvalid ? key : 0)) * ldk + (int64_t)hkv * D, kvalid, lane, kf);
    const bool kvis = kvalid && (key_mask == nullptr || key_mask[tok0 + key] != 0);
    const float scale_log2 = scale * LOG2E, inv_h = 1.f / (float)Hq;
    f32x16 adk[C::DT];
    zero_tiles(adk);
    const int qt0 = (kb * 128) / 32;
    const int nqt = (S + 31) / 32;
    for (int hq = hkv * rep; hq < (hkv + 1) * rep; ++hq) {
        for (int qt = qt0; qt < nqt; ++qt) {
            const int qs = qt * 32;
            __syncthreads();
            load_tile<D, 256>(qimg, q + (tok0 + qs) * ldq + (int64_t)hq * D, ldq, S - qs, threadIdx.x);
            if (threadIdx.x < 32) {
                const bool okq = qs + threadIdx.x < S;
                stat[0][threadIdx.x] = okq ? lse[((int64_t)b * Hq + hq) * S + qs + threadIdx.x] * LOG2E : 0.f;
                stat[1][threadIdx.x] = okq ? delta[((int64_t)b * Hq + hq) * S + qs + threadIdx.x] : 0.f;
            }
            __syncthreads();
            if (qs + 31 < k0) continue;  // every query of the tile precedes this wave's keys
            f32x16 s;
            zero_tile(s);
            mma_rows<D>(s, qimg, kf, lane);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = acc_row(i, lane);
                const int qi = qs + r;
                const bool ok = kvis && qi < S && key <= qi;
                const float p = ok ? exp2f(s[i] * scale_log2 - stat[0][r]) : 0.f;
                const float g = (ok && key < qi) ? da[(tok0 + qi) * S + key] : 0.f;
                s[i] = p * (g * inv_h - stat[1][r]) * scale;
            }
            const bf16x8 d0 = pack_frag(s, 0), d1 = pack_frag(s, 1);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) mma_cols<D>(adk[dt], qimg, 32 * dt, d0, d1, lane);
        }
    }
    store_t_tiles<C::DT>(adk, 1.f, dk + (tok0 + key) * lddk + (int64_t)hkv * D, kvalid, lane);
}

// ------------------------------------------------------------------------------------------------ prepare from materialised weights
__device__ __forceinline__ float ral_ld(const float* p) { return *p; }
__device__ __forceinline__ float ral_ld(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ void ral_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void ral_st(bf16_t* p, float v) { *p = f2bf(v); }

// a(i, j) of row (b, i): the mean over the heads in head order, the diagonal 0
template <class T>
__device__ __forceinline__ float ral_head_mean(const T* __restrict__ wrow, int64_t head_stride, int H, int i, int j) {
    float a = 0.f;
    for (int h = 0; h < H; ++h) a += ral_ld(wrow + h * head_stride + j);
    return j == i ? 0.f : a / (float)H;
}

// one wave per row (b, i) of weights [B, H, S, S]; no causal assumption: the reference masks the diagonal only
template <class T>
__global__ __launch_bounds__(256) void ral_prepare_fwd_kernel(int64_t rows, int H, int S, const T* __restrict__ w, float* __restrict__ P, float* __restrict__ Z) {
    const int lane = threadIdx.x & 63;
    const int64_t ss = (int64_t)S * S;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int64_t b = row / S;
        const int i = (int)(row % S);
        const T* wrow = w + b * H * ss + (int64_t)i * S;
        float sum = 0.f;
        for (int j = lane; j < S; j += 64) sum += ral_head_mean(wrow, ss, H, i, j);
        const float zc = fmaxf(wave_sum(sum), RAL_EPS);
        for (int j = lane; j < S; j += 64) P[row * S + j] = fmaxf(ral_head_mean(wrow, ss, H, i, j) / zc, RAL_EPS);
        if (lane == 0) Z[row] = zc;
    }
}

// dweights[b, h, i, j] = da[b, i, j] / H (da holds 0 on the diagonal)
template <class T>
__global__ __launch_bounds__(256) void ral_prepare_bwd_kernel(int64_t total, int H, int S, const float* __restrict__ da, T* __restrict__ dw) {
    const int64_t ss = (int64_t)S * S;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / (ss * H);
        ral_st(dw + e, da[b * ss + e % ss] / (float)H);
    }
}

// The backward of a -> P = clamp(a / clamp(sum a, 1e-8), 1e-8), as autograd of the reference yields it.  u = "the entry is not clamped" (P > 1e-8):
//   da(i,j) = (u dP(i,j) - sum_j' u dP P) / Z(i);  where Z itself is clamped the sum has no gradient: no row term, and 1 / 1e-8 as the factor.
// causal = 0: the diagonal is written as 0 (the reference's masked_fill); causal = 1: everything on and above it (the q, k path: a is a constant 0 there).
__global__ __launch_bounds__(256) void ral_renorm_bwd_kernel(int64_t rows, int S, const float* __restrict__ P, const float* __restrict__ Z,
                                                             const float* __restrict__ dP, int causal, float* __restrict__ da) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const int i = (int)(row % S);
        const float zc = Z[row];
        const float* pr = P + row * S;
        const float* gr = dP + row * S;
        float t = 0.f;
        if (zc > RAL_EPS) {
            for (int j = lane; j < S; j += 64) t += pr[j] > RAL_EPS ? gr[j] * pr[j] : 0.f;
            t = wave_sum(t);
        }
        for (int j = lane; j < S; j += 64) {
            const float v = ((pr[j] > RAL_EPS ? gr[j] : 0.f) - t) / zc;
            da[row * S + j] = (causal ? j >= i : j == i) ? 0.f : v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ JSD rows and the reduction
// jsd[b, i] = 0.5 sum_j (P log(P / M) + Q log(Q / M)), M = (P + Q) / 2.  P = Q = 1e-8 gives M = 1e-8 and log(1) = 0: exactly 0.
__global__ __launch_bounds__(256) void ral_jsd_fwd_kernel(int64_t rows, int S, const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ jsd) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        float acc = 0.f;
        for (int j = lane; j < S; j += 64) {
            const float p = P[row * S + j], qv = Q[row * S + j];
            const float m = (p + qv) * 0.5f;
            acc += p * logf(p / m) + qv * logf(qv / m);
        }
        acc = wave_sum(acc);
        if (lane == 0) jsd[row] = 0.5f * acc;
    }
}

// dP(i, j) = 0.5 w(b, i) log(P / M)
__global__ __launch_bounds__(256) void ral_jsd_bwd_kernel(int64_t rows, int S, const float* __restrict__ P, const float* __restrict__ Q,
                                                          const float* __restrict__ w, float* __restrict__ dP) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const float hw = 0.5f * w[row];
        for (int j = lane; j < S; j += 64) {
            const float p = P[row * S + j];
            dP[row * S + j] = hw * logf(p / ((p + Q[row * S + j]) * 0.5f));
        }
    }
}

// loss = factor * mean_b (adv_b * sum_i jsd mask / max(sum_i mask, 1));  w[b, i] = g * factor / B * adv_b * mask[b, i] / max(sum_i mask, 1), g = *grad
// (1 if NULL): the derivative of the loss with respect to jsd[b, i] times the incoming scalar gradient, which stays on the device.  One workgroup,
// a wave per sample, the samples folded in a fixed order.
__global__ __launch_bounds__(256) void ral_reduce_kernel(int B, int S, const float* __restrict__ jsd, const float* __restrict__ adv,
                                                         const float* __restrict__ mask, float factor, const float* __restrict__ grad,
                                                         float* __restrict__ loss, float* __restrict__ w) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float g = (grad ? *grad : 1.f) * factor / (float)B;
    float acc = 0.f;
    for (int b = wave; b < B; b += 4) {
        const float* jr = jsd + (int64_t)b * S;
        const float* mr = mask + (int64_t)b * S;
        float cnt = 0.f, num = 0.f;
        for (int i = lane; i < S; i += 64) {
            cnt += mr[i];
            num += jr[i] * mr[i];
        }
        cnt = wave_sum(cnt);
        num = wave_sum(num);
        const float den = fmaxf(cnt, 1.f);
        acc += adv[b] * num / den;
        if (w) {
            const float gb = g * adv[b] / den;
            for (int i = lane; i < S; i += 64) w[(int64_t)b * S + i] = gb * mr[i];
        }
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && loss) *loss = factor * ((part[0] + part[1] + part[2] + part[3]) / (float)B);
}

// dst = bf16(a + b): the gradients that arrive on the exposed q, k join dq, dk ahead of the RoPE backward
__global__ __launch_bounds__(256) void ral_add_bf16_kernel(int64_t n, const bf16_t* __restrict__ a, const bf16_t* __restrict__ b, bf16_t* __restrict__ dst) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = f2bf(bf2f(a[i]) + bf2f(b[i]));
}

// ------------------------------------------------------------------------------------------------ host checks
int check_qk(const char* who, int B, int S, int Hq, int Hkv, int D, int64_t ldq, int64_t ldk) {
    MI355_REQUIRE(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "%s: query heads (%d) must be a multiple of kv heads (%d)", who, Hq, Hkv);
    MI355_REQUIRE(D == 64 || D == 128, "%s: head_dim %d not built (64, 128)", who, D);
    MI355_REQUIRE(B >= 0 && S >= 0, "%s: negative batch or sequence length", who);
    MI355_REQUIRE(B <= 65535 && Hq <= 65535 && S <= (1 << 30) - 64, "%s: grid limits (B, Hq <= 65535, S <= 2^30 - 64)", who);
    MI355_REQUIRE(ldq >= (int64_t)Hq * D && ldk >= (int64_t)Hkv * D, "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0, "%s: leading dimensions must be multiples of 8 elements", who);
    return 0;
}

int check_rows(const char* who, int B, int S) {
    MI355_REQUIRE(B >= 0 && S >= 0 && S <= (1 << 30), "%s: bad batch (%d) or sequence length (%d)", who, B, S);
    return 0;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" int mi355_ral_qk_prepare_fwd(int B, int S, int Hq, int Hkv, int D, const void* q, int64_t ldq, const void* k, int64_t ldk, const uint8_t* key_mask,
                                        float scale, float* P, float* Z, float* lse, void* stream) {
    if (check_qk("mi355_ral_qk_prepare_fwd", B, S, Hq, Hkv, D, ldq, ldk)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(q && k && P && Z && lse, "mi355_ral_qk_prepare_fwd: null pointer");
    MI355_REQUIRE(aligned16({q, k}), "mi355_ral_qk_prepare_fwd: q, k must be 16-byte aligned");
    MI355_REQUIRE((((uintptr_t)P | (uintptr_t)Z | (uintptr_t)lse) & 3) == 0, "mi355_ral_qk_prepare_fwd: P, Z, lse must be 4-byte aligned");
    const dim3 grid((S + 127) / 128, B);
    if (D == 64) ral_qk_fwd_kernel<64><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale * LOG2E, P, Z, lse);
    else ral_qk_fwd_kernel<128><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale * LOG2E, P, Z, lse);
    MI355_LAUNCH_CHECK("mi355_ral_qk_prepare_fwd");
    return 0;
}

extern "C" int mi355_ral_qk_prepare_bwd(int B, int S, int Hq, int Hkv, int D, const void* q, int64_t ldq, const void* k, int64_t ldk, const uint8_t* key_mask,
                                        float scale, const float* da, const float* lse, float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk,
                                        void* stream) {
    if (check_qk("mi355_ral_qk_prepare_bwd", B, S, Hq, Hkv, D, ldq, ldk)) return 1;
    if (check_qk("mi355_ral_qk_prepare_bwd", B, S, Hq, Hkv, D, lddq, lddk)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(q && k && da && lse && delta && dq && dk, "mi355_ral_qk_prepare_bwd: null pointer");
    MI355_REQUIRE(aligned16({q, k, dq, dk}), "mi355_ral_qk_prepare_bwd: q, k, dq, dk must be 16-byte aligned");
    MI355_REQUIRE((((uintptr_t)da | (uintptr_t)lse | (uintptr_t)delta) & 3) == 0, "mi355_ral_qk_prepare_bwd: da, lse, delta must be 4-byte aligned");
    const dim3 gq((S + 127) / 128, Hq, B), gk((S + 127) / 128, Hkv, B);
#define LAUNCH(DD)                                                                                                                                      \
    do {                                                                                                                                                \
        ral_qk_bwd_dq_kernel<DD><<<gq, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale, da, lse, delta, \
                                                             (bf16_t*)dq, lddq);                                                                        \
        ral_qk_bwd_dk_kernel<DD><<<gk, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale, da, lse, delta, \
                                                             (bf16_t*)dk, lddk);                                                                        \
    } while (0)
    if (D == 64) LAUNCH(64); else LAUNCH(128);
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_ral_qk_prepare_bwd");
    return 0;
}

extern "C" int mi355_ral_prepare_fwd(int B, int H, int S, const void* weights, int dtype, float* P, float* Z, void* stream) {
    if (check_rows("mi355_ral_prepare_fwd", B, S)) return 1;
    MI355_REQUIRE(H > 0, "mi355_ral_prepare_fwd: bad head count %d", H);
    MI355_REQUIRE(dtype == MI355_DT_BF16 || dtype == MI355_DT_F32, "mi355_ral_prepare_fwd: dtype %d (bf16 or fp32)", dtype);
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(weights && P && Z, "mi355_ral_prepare_fwd: null pointer");
    MI355_REQUIRE(((uintptr_t)weights & (dtype == MI355_DT_F32 ? 3 : 1)) == 0 && (((uintptr_t)P | (uintptr_t)Z) & 3) == 0, "mi355_ral_prepare_fwd: misaligned pointer");
    const int64_t rows = (int64_t)B * S;
    if (dtype == MI355_DT_F32) ral_prepare_fwd_kernel<float><<<row_grid(rows), 256, 0, ST(stream)>>>(rows, H, S, (const float*)weights, P, Z);
    else ral_prepare_fwd_kernel<bf16_t><<<row_grid(rows), 256, 0, ST(stream)>>>(rows, H, S, (const bf16_t*)weights, P, Z);
    MI355_LAUNCH_CHECK("mi355_ral_prepare_fwd");
    return 0;
}

extern "C" int mi355_ral_prepare_bwd(int B, int H, int S, const float* da, void* dweights, int dtype, void* stream) {
    if (check_rows("mi355_ral_prepare_bwd", B, S)) return 1;
    MI355_REQUIRE(H > 0, "mi355_ral_prepare_bwd: bad head count %d", H);
    MI355_REQUIRE(dtype == MI355_DT_BF16 || dtype == MI355_DT_F32, "mi355_ral_prepare_bwd: dtype %d (bf16 or fp32)", dtype);
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(da && dweights, "mi355_ral_prepare_bwd: null pointer");
    MI355_REQUIRE(((uintptr_t)dweights & (dtype == MI355_DT_F32 ? 3 : 1)) == 0 && ((uintptr_t)da & 3) == 0, "mi355_ral_prepare_bwd: misaligned pointer");
    const int64_t total = (int64_t)B * H * S * S;
    if (dtype == MI355_DT_F32) ral_prepare_bwd_kernel<float><<<flat_grid(total), 256, 0, ST(stream)>>>(total, H, S, da, (float*)dweights);
    else ral_prepare_bwd_kernel<bf16_t><<<flat_grid(total), 256, 0, ST(stream)>>>(total, H, S, da, (bf16_t*)dweights);
    MI355_LAUNCH_CHECK("mi355_ral_prepare_bwd");
    return 0;
}

extern "C" int mi355_ral_renorm_bwd(int B, int S, const float* P, const float* Z, const float* dP, int causal, float* da, void* stream) {
    if (check_rows("mi355_ral_renorm_bwd", B, S)) return 1;
    MI355_REQUIRE(causal == 0 || causal == 1, "mi355_ral_renorm_bwd: causal %d (0 or 1)", causal);
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(P && Z && dP && da, "mi355_ral_renorm_bwd: null pointer");
    MI355_REQUIRE((((uintptr_t)P | (uintptr_t)Z | (uintptr_t)dP | (uintptr_t)da) & 3) == 0, "mi355_ral_renorm_bwd: misaligned pointer");
    const int64_t rows = (int64_t)B * S;
    ral_renorm_bwd_kernel<<<row_grid(rows), 256, 0, ST(stream)>>>(rows, S, P, Z, dP, causal, da);
    MI355_LAUNCH_CHECK("mi355_ral_renorm_bwd");
    return 0;
}

extern "C" int mi355_ral_jsd_fwd(int B, int S, const float* P, const float* Q, float* jsd, void* stream) {
    if (check_rows("mi355_ral_jsd_fwd", B, S)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(P && Q && jsd, "mi355_ral_jsd_fwd: null pointer");
    MI355_REQUIRE((((uintptr_t)P | (uintptr_t)Q | (uintptr_t)jsd) & 3) == 0, "mi355_ral_jsd_fwd: misaligned pointer");
    const int64_t rows = (int64_t)B * S;
    ral_jsd_fwd_kernel<<<row_grid(rows), 256, 0, ST(stream)>>>(rows, S, P, Q, jsd);
    MI355_LAUNCH_CHECK("mi355_ral_jsd_fwd");
    return 0;
}

extern "C" int mi355_ral_jsd_bwd(int B, int S, const float* P, const float* Q, const float* w, float* dP, void* stream) {
    if (check_rows("mi355_ral_jsd_bwd", B, S)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(P && Q && w && dP, "mi355_ral_jsd_bwd: null pointer");
    MI355_REQUIRE((((uintptr_t)P | (uintptr_t)Q | (uintptr_t)w | (uintptr_t)dP) & 3) == 0, "mi355_ral_jsd_bwd: misaligned pointer");
    const int64_t rows = (int64_t)B * S;
    ral_jsd_bwd_kernel<<<row_grid(rows), 256, 0, ST(stream)>>>(rows, S, P, Q, w, dP);
    MI355_LAUNCH_CHECK("mi355_ral_jsd_bwd");
    return 0;
}

extern "C" int mi355_ral_reduce(int B, int S, const float* jsd, const float* advantages, const float* loss_mask, float ral_factor, const float* grad,
                                float* loss, float* w, void* stream) {
    MI355_REQUIRE(B > 0 && S > 0 && S <= (1 << 30), "mi355_ral_reduce: bad batch (%d) or sequence length (%d)", B, S);
    MI355_REQUIRE(jsd && advantages && loss_mask && (loss || w), "mi355_ral_reduce: null pointer");
    MI355_REQUIRE((((uintptr_t)jsd | (uintptr_t)advantages | (uintptr_t)loss_mask | (uintptr_t)grad | (uintptr_t)loss | (uintptr_t)w) & 3) == 0,
                  "mi355_ral_reduce: misaligned pointer");
    ral_reduce_kernel<<<1, 256, 0, ST(stream)>>>(B, S, jsd, advantages, loss_mask, ral_factor, grad, loss, w);
    MI355_LAUNCH_CHECK("mi355_ral_reduce");
    return 0;
}

extern "C" int mi355_ral_add_bf16(int64_t n, const void* a, const void* b, void* dst, void* stream) {
    MI355_REQUIRE(n >= 0 && n <= ((int64_t)1 << 40), "mi355_ral_add_bf16: bad element count");
    if (n == 0) return 0;
    MI355_REQUIRE(a && b && dst, "mi355_ral_add_bf16: null pointer");
    MI355_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)dst) & 1) == 0, "mi355_ral_add_bf16: misaligned pointer");
    ral_add_bf16_kernel<<<flat_grid(n), 256, 0, ST(stream)>>>(n, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)dst);
    MI355_LAUNCH_CHECK("mi355_ral_add_bf16");
    return 0;
}
