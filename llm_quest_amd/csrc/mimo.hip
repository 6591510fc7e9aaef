// MiMo-V2-Flash (reference xiaomi/): attention with a learnable sink and decoupled q/k and v head dims, the sink's gradient, and the per-head
// RMSNorm + partial RoPE of the q and k heads.
//
// Sink attention (mimo_v2_flash_attention.py:100-130, where it is a dense masked score matrix with one extra column per head):
//   allowed(i, j) = i - W < j <= i,  W >= 1 (W >= S: plain causal, the GA layers);  s_ij = scale * q_i . k_j over D features;
//   p_ij = exp(s_ij - m_i) / (sum_j exp(s_ij - m_i) + exp(z_h - m_i));  o_i = sum_j p_ij v_j over DV features;  lse_i = log(sum_j exp(s_ij) + exp(z_h)).
// The sink logit z_h is NOT multiplied by the scale and has no value row.  The kernels are the three of gemma3.hip -- S^T = K Q^T with the query on
// the MFMA lane, lane-local online softmax, only the key tiles that meet the band are walked, a query-major dQ pass and a key-major dK/dV pass,
// no atomics -- with two differences: the k image and the v image have their own widths (<D, DV>), and the sink joins the online softmax as one more
// key without a value: the state (m, l, acc) of the tile loop is merged with (z_h log2(e), 1, 0) once, behind the loop (a NULL sink: no merge).  In the
// backward delta_i = sum_d dO_i O_i is unchanged (the sink's value is zero) and p is recomputed from the saved lse, which already holds the sink.
//
// Sink gradient: dz_h = - sum_{b,i} exp(z_h - lse[b,h,i]) delta[b,h,i], per-workgroup partial rows [parts, Hq] for mi355_reduce_rows_f32.
//
// Norm + partial RoPE (mimo_v2_flash_attention.py:88-94): n = x rsqrt(mean(x^2) + eps) w over head_dim (torch.nn.RMSNorm in fp32), then the half-split
// rotation of the first R features, pairs (d, d + R/2), cos / sin rounded to bf16; features >= R pass through.  One wave per (token, head) row,
// fp32 math, one rounding at the output; R is any even number in [2, D].
#include <initializer_list>

#include "attn_tile32.h"
#include "rows_bf16.h"

namespace {

// ------------------------------------------------------------------------------------------------ sink attention, forward
// W is already clamped to [1, S] and S <= 2^30 - 64 (check_sink): every sum of an index and W below stays inside int.
template <int D, int DV>
__global__ __launch_bounds__(256) void sink_fwd_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
                                                       const bf16_t* __restrict__ k, int64_t ldk, const bf16_t* __restrict__ v, int64_t ldv,
                                                       const float* __restrict__ sink, bf16_t* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                                       float scale_log2) {
    using CK = Tile32<D>;
    using CV = Tile32<DV>;
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    char* kimg = smem;
    char* vimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hkv = h / (Hq / Hkv);
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 qf[CK::KS];
    load_row_frags<D>(q + (tok0 + query) * ldq + (int64_t)h * D, qvalid, lane, qf);
    f32x16 acc[CV::DT];
#pragma unroll
    for (int dt = 0; dt < CV::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
    float m = NEG_INF, l = 0.f;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    const int kfirst = qb - W + 1 > 0 ? qb - W + 1 : 0;  // first key of the workgroup's first query's window
    for (int kt = kfirst / 32; kt <= qlast / 32; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
        load_tile<DV, 256>(vimg, v + (tok0 + key0) * ldv + (int64_t)hkv * DV, ldv, S - key0, threadIdx.x);
        __syncthreads();
        // tile above this wave's diagonal, or wholly before the window of its first query (later queries' windows start later still)
        if (q0 >= S || key0 > q0 + 31 || key0 + 31 + W <= q0) continue;
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < CK::KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(kimg, ks, lane), qf[ks], s, 0, 0, 0);
        float mx = NEG_INF;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            const bool ok = key < S && key <= query && key + W > query;
            s[i] = ok ? s[i] * scale_log2 : NEG_INF;
            mx = fmaxf(mx, s[i]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m, mx);
        const float m_use = m_new == NEG_INF ? 0.f : m_new;  // a row whose window this tile does not reach yet
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
        for (int dt = 0; dt < CV::DT; ++dt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[dt][i] *= alpha;
        const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CV::DT; ++dt) {
            acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<DV>(vimg, 32 * dt, 0, lane), p0, acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<DV>(vimg, 32 * dt, 16, lane), p1, acc[dt], 0, 0, 0);
        }
    }
    // the sink: one more "key" of logit z_h whose value row is zero, merged into the state (m, l, acc) like a last tile.  (Merged first, as the initial
    // state m = z_h log2 e, l = 1, the algebra is the same, but the compiler then holds the accumulators twice -- 62 AGPRs instead of 32 at (64, 64), a wave
    // per SIMD fewer -- and the forward is a third slower.)  A sink far below every score leaves m, l and the scale 1 / l exactly as they were.
    float mul = 1.f / l;
    if (sink) {
        const float z2 = sink[h] * LOG2E;
        const float m_new = fmaxf(m, z2);
        const float alpha = exp2f(m - m_new);  // 0 for a row past S, whose m is still -inf
        l = l * alpha + exp2f(z2 - m_new);
        m = m_new;
        mul = alpha / l;
    }
    store_t_tiles<CV::DT>(acc, mul, o + (tok0 + query) * ldo + (int64_t)h * DV, qvalid, lane);
    if (lane < 32 && qvalid) lse[((int64_t)b * Hq + h) * S + query] = (m + log2f(l)) * LN2;
}

// ------------------------------------------------------------------------------------------------ dQ pass (query-major, the forward's band)
template <int D, int DV>
__global__ __launch_bounds__(256) void sink_bwd_dq_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
                                                          const bf16_t* __restrict__ k, int64_t ldk, const bf16_t* __restrict__ v, int64_t ldv,
                                                          const bf16_t* __restrict__ d_o, int64_t lddo, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, bf16_t* __restrict__ dq, int64_t lddq, float scale) {
    using CK = Tile32<D>;
    using CV = Tile32<DV>;
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    char* kimg = smem;
    char* vimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hkv = h / (Hq / Hkv);
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 qf[CK::KS], gf[CV::KS];
    load_row_frags<D>(q + (tok0 + query) * ldq + (int64_t)h * D, qvalid, lane, qf);
    load_row_frags<DV>(d_o + (tok0 + query) * lddo + (int64_t)h * DV, qvalid, lane, gf);
    const float lse_q = qvalid ? lse[((int64_t)b * Hq + h) * S + query] * LOG2E : 0.f;
    const float delta_q = qvalid ? delta[((int64_t)b * Hq + h) * S + query] : 0.f;
    const float scale_log2 = scale * LOG2E;
    f32x16 acc[CK::DT];
#pragma unroll
    for (int dt = 0; dt < CK::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[dt][i] = 0.f;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    const int kfirst = qb - W + 1 > 0 ? qb - W + 1 : 0;
    for (int kt = kfirst / 32; kt <= qlast / 32; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
        load_tile<DV, 256>(vimg, v + (tok0 + key0) * ldv + (int64_t)hkv * DV, ldv, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31 || key0 + 31 + W <= q0) continue;
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < CK::KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(kimg, ks, lane), qf[ks], s, 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < CV::KS; ++ks) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DV>(vimg, ks, lane), gf[ks], dp, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
            const bool ok = qvalid && key <= query && key + W > query;
            const float p = ok ? exp2f(s[i] * scale_log2 - lse_q) : 0.f;
            s[i] = p * (dp[i] - delta_q) * scale;
        }
        const bf16x8 d0 = pack_frag(s, 0), d1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CK::DT; ++dt) {
            acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(kimg, 32 * dt, 0, lane), d0, acc[dt], 0, 0, 0);
            acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(kimg, 32 * dt, 16, lane), d1, acc[dt], 0, 0, 0);
        }
    }
    store_t_tiles<CK::DT>(acc, 1.f, dq + (tok0 + query) * lddq + (int64_t)h * D, qvalid, lane);
}

// ------------------------------------------------------------------------------------------------ dK/dV pass (key-major)
// A wave owns 32 keys of one kv head; all q heads of the group and the query tiles kb .. min(S - 1, k_last + W - 1) are walked.
template <int D, int DV>
__global__ __launch_bounds__(256) void sink_bwd_dkv_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
                                                           const bf16_t* __restrict__ k, int64_t ldk, const bf16_t* __restrict__ v, int64_t ldv,
                                                           const bf16_t* __restrict__ d_o, int64_t lddo, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, bf16_t* __restrict__ dk, int64_t lddk,
                                                           bf16_t* __restrict__ dv, int64_t lddv, float scale) {
    using CK = Tile32<D>;
    using CV = Tile32<DV>;
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    __shared__ float stat[2][32];
    char* qimg = smem;
    char* gimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, hkv = blockIdx.y, rep = Hq / Hkv;
    const int kb = blockIdx.x * 128;
    const int k0 = kb + wave * 32;
    const int key = k0 + (lane & 31);
    const bool kvalid = key < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 kf[CK::KS], vf[CV::KS];
    load_row_frags<D>(k + (tok0 + key) * ldk + (int64_t)hkv * D, kvalid, lane, kf);
    load_row_frags<DV>(v + (tok0 + key) * ldv + (int64_t)hkv * DV, kvalid, lane, vf);
    const float scale_log2 = scale * LOG2E;
    f32x16 adk[CK::DT], adv[CV::DT];
#pragma unroll
    for (int dt = 0; dt < CK::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) adk[dt][i] = 0.f;
#pragma unroll
    for (int dt = 0; dt < CV::DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) adv[dt][i] = 0.f;
    const int klast = (kb + 127 < S ? kb + 127 : S - 1);
    const int qend = (klast + W - 1 < S - 1 ? klast + W - 1 : S - 1);  // last query that sees a key of this workgroup
    for (int hq = hkv * rep; hq < (hkv + 1) * rep; ++hq) {
        for (int qt = kb / 32; qt <= qend / 32; ++qt) {
            const int qs = qt * 32;
            __syncthreads();
            load_tile<D, 256>(qimg, q + (tok0 + qs) * ldq + (int64_t)hq * D, ldq, S - qs, threadIdx.x);
            load_tile<DV, 256>(gimg, d_o + (tok0 + qs) * lddo + (int64_t)hq * DV, lddo, S - qs, threadIdx.x);
            if (threadIdx.x < 32) {
                const bool okq = qs + threadIdx.x < S;
                stat[0][threadIdx.x] = okq ? lse[((int64_t)b * Hq + hq) * S + qs + threadIdx.x] * LOG2E : 0.f;
                stat[1][threadIdx.x] = okq ? delta[((int64_t)b * Hq + hq) * S + qs + threadIdx.x] : 0.f;
            }
            __syncthreads();
            // every query of the tile precedes this wave's keys, or the tile starts past the window of its last key
            if (k0 >= S || qs + 31 < k0 || qs >= k0 + 31 + W) continue;
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < CK::KS; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(qimg, ks, lane), kf[ks], s, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < CV::KS; ++ks) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<DV>(gimg, ks, lane), vf[ks], dp, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3);
                const int qi = qs + r;
                const bool ok = kvalid && qi < S && key <= qi && key + W > qi;
                const float p = ok ? exp2f(s[i] * scale_log2 - stat[0][r]) : 0.f;
                s[i] = p;
                dp[i] = p * (dp[i] - stat[1][r]) * scale;
            }
            const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1), d0 = pack_frag(dp, 0), d1 = pack_frag(dp, 1);
#pragma unroll
            for (int dt = 0; dt < CV::DT; ++dt) {
                adv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<DV>(gimg, 32 * dt, 0, lane), p0, adv[dt], 0, 0, 0);
                adv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<DV>(gimg, 32 * dt, 16, lane), p1, adv[dt], 0, 0, 0);
            }
#pragma unroll
            for (int dt = 0; dt < CK::DT; ++dt) {
                adk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(qimg, 32 * dt, 0, lane), d0, adk[dt], 0, 0, 0);
                adk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_cols<D>(qimg, 32 * dt, 16, lane), d1, adk[dt], 0, 0, 0);
            }
        }
    }
    store_t_tiles<CK::DT>(adk, 1.f, dk + (tok0 + key) * lddk + (int64_t)hkv * D, kvalid, lane);
    store_t_tiles<CV::DT>(adv, 1.f, dv + (tok0 + key) * lddv + (int64_t)hkv * DV, kvalid, lane);
}

// ------------------------------------------------------------------------------------------------ sink gradient
// partial[wg, h] = - sum over this workgroup's (b, i) of exp(z_h - lse[b, h, i]) delta[b, h, i]; lanes, waves and workgroups are folded in a fixed order.
__global__ __launch_bounds__(256) void sink_grad_kernel(int B, int S, int Hq, const float* __restrict__ sink, const float* __restrict__ lse,
                                                        const float* __restrict__ delta, float* __restrict__ partial) {
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t n = (int64_t)B * S;
    for (int h = 0; h < Hq; ++h) {
        const float z = sink[h];
        float acc = 0.f;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            const int64_t bb = i / S;
            const int64_t idx = (bb * Hq + h) * S + (i - bb * S);
            acc += expf(z - lse[idx]) * delta[idx];  // lse >= z: the exponent is never positive
        }
        acc = wave_sum(acc);
        __syncthreads();
        if (lane == 0) red[wv] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * Hq + h] = -(((red[0] + red[1]) + red[2]) + red[3]);
    }
}

// ------------------------------------------------------------------------------------------------ per-head RMSNorm + partial RoPE
// A row is one (token, head), head < Hq a query head, else a key head; lane owns features lane, lane + 64, ..  The rotation partner of feature d
// (d +- R/2) is read from x again and normalised with the row's factor, so no lane exchanges values and R needs no alignment.
template <int D, bool BWD>
__global__ __launch_bounds__(256) void mimo_normrope_kernel(int64_t tokens, int S, int Hq, int Hkv, int R, const bf16_t* __restrict__ x, int64_t ldx,
                                                            const bf16_t* __restrict__ qw, const bf16_t* __restrict__ kw,
                                                            const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                            const bf16_t* __restrict__ dy, int64_t lddy, bf16_t* __restrict__ out, int64_t ldo,
                                                            float* __restrict__ partial, float eps) {
    constexpr int NE = (D + 63) / 64;
    __shared__ float acc_lds[4][2][D];  // [wave][q weight, k weight][feature]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int H = Hq + Hkv, half = R >> 1;
    const int64_t total = tokens * H;
    float wq[NE], wk[NE], wqp[NE], wkp[NE], g_acc[2][NE];
    int partner[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        const int d = lane + 64 * e;
        const bool in = d < D;
        partner[e] = (in && d < R) ? (d < half ? d + half : d - half) : -1;
        wq[e] = in ? bf2f(qw[d]) : 0.f;
        wk[e] = in ? bf2f(kw[d]) : 0.f;
        wqp[e] = partner[e] >= 0 ? bf2f(qw[partner[e]]) : 0.f;
        wkp[e] = partner[e] >= 0 ? bf2f(kw[partner[e]]) : 0.f;
        g_acc[0][e] = g_acc[1][e] = 0.f;
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < total; row += (int64_t)gridDim.x * 4) {
        const int64_t t = row / H;
        const int h = (int)(row % H);
        const bool is_q = h < Hq;
        const int pos = (int)(t % S);
        const bf16_t* xr = x + t * ldx + (int64_t)h * D;
        float xv[NE], ss = 0.f;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int d = lane + 64 * e;
            xv[e] = d < D ? bf2f(xr[d]) : 0.f;
            ss += xv[e] * xv[e];
        }
        const float a = rsqrtf(wave_sum(ss) / (float)D + eps);
        if (!BWD) {
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int d = lane + 64 * e;
                if (d >= D) continue;
                float y = xv[e] * a * (is_q ? wq[e] : wk[e]);
                if (partner[e] >= 0) {
                    const float np = bf2f(xr[partner[e]]) * a * (is_q ? wqp[e] : wkp[e]);
                    const float c = rbf(cos_t[(int64_t)pos * R + d]), s = rbf(sin_t[(int64_t)pos * R + d]);
                    y = d < half ? c * y - s * np : c * y + s * np;  // cos * n + sin * cat(-n2, n1)
                }
                out[t * ldo + (int64_t)h * D + d] = f2bf(y);
            }
        } else {
            // the adjoint of the rotation, then y = x a w:  dx = a g - a^3 x <g, x> / D, g = w dn;  dw = sum over rows of dn x a
            const bf16_t* dyr = dy + t * lddy + (int64_t)h * D;
            float g[NE], dn[NE], dot = 0.f;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int d = lane + 64 * e;
                dn[e] = d < D ? bf2f(dyr[d]) : 0.f;
                if (partner[e] >= 0) {
                    const float c = rbf(cos_t[(int64_t)pos * R + d]), sp = rbf(sin_t[(int64_t)pos * R + partner[e]]);
                    const float dp = bf2f(dyr[partner[e]]);
                    dn[e] = d < half ? c * dn[e] + sp * dp : c * dn[e] - sp * dp;
                }
                g[e] = dn[e] * (is_q ? wq[e] : wk[e]);
                dot += g[e] * xv[e];
            }
            const float coef = a * a * a * wave_sum(dot) / (float)D;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int d = lane + 64 * e;
                if (d >= D) continue;
                out[t * ldo + (int64_t)h * D + d] = f2bf(a * g[e] - coef * xv[e]);
                g_acc[is_q ? 0 : 1][e] += dn[e] * xv[e] * a;
            }
        }
    }
    if (BWD) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int d = lane + 64 * e;
            if (d < D) {
                acc_lds[wv][0][d] = g_acc[0][e];
                acc_lds[wv][1][d] = g_acc[1][e];
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 2 * D; i += 256)
            partial[(int64_t)blockIdx.x * 2 * D + i] = ((acc_lds[0][i / D][i % D] + acc_lds[1][i / D][i % D]) + acc_lds[2][i / D][i % D]) + acc_lds[3][i / D][i % D];
    }
}

// ------------------------------------------------------------------------------------------------ host checks
// the kernels move 16 bytes at a time: every operand pointer must be 16-byte aligned (NULL passes here and is refused by the null check)
bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}

// (192, 128) is the released model's pair: its three kernels need no scratch (dK/dV: 212 VGPRs + 192 AGPRs at one wave per SIMD)
#define MIMO_PAIRS(X) X(64, 32) X(64, 64) X(128, 64) X(128, 128) X(192, 128)
#define MIMO_PAIR_NAMES "(64, 32), (64, 64), (128, 64), (128, 128), (192, 128)"

bool pair_built(int D, int DV) {
#define X(DD, VV) \
    if (D == DD && DV == VV) return true;
    MIMO_PAIRS(X)
#undef X
    return false;
}

int check_sink(const char* who, int B, int S, int Hq, int Hkv, int D, int DV, int W, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo) {
    MI355_REQUIRE(B >= 0 && S >= 0, "%s: negative batch or sequence length", who);
    MI355_REQUIRE(W >= 1, "%s: window %d must be at least 1", who, W);
    MI355_REQUIRE(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "%s: query heads (%d) must be a multiple of kv heads (%d)", who, Hq, Hkv);
    MI355_REQUIRE(pair_built(D, DV), "%s: (head_dim, value_head_dim) = (%d, %d) not built " MIMO_PAIR_NAMES, who, D, DV);
    MI355_REQUIRE(ldq >= (int64_t)Hq * D && ldo >= (int64_t)Hq * DV && ldk >= (int64_t)Hkv * D && ldv >= (int64_t)Hkv * DV,
                  "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "%s: leading dimensions must be multiples of 8 elements", who);
    // S <= 2^30 - 64: with W clamped to S the largest index sum in the kernels, k0 + 31 + W < 2 S + 32, stays inside int
    MI355_REQUIRE(B <= 65535 && Hq <= 65535 && S <= (1 << 30) - 64, "%s: grid limits (B, Hq <= 65535, S <= 2^30 - 64)", who);
    return 0;
}

int check_normrope(const char* who, int64_t tokens, int S, int Hq, int Hkv, int D, int R, int64_t ldx, int64_t ldy, int64_t table_rows) {
    MI355_REQUIRE(tokens >= 0 && tokens <= ((int64_t)1 << 40) && S > 0 && Hq >= 0 && Hkv >= 0 && Hq <= 65535 && Hkv <= 65535 && Hq + Hkv > 0,
                  "%s: bad token / head counts", who);
    MI355_REQUIRE(D == 64 || D == 128 || D == 192, "%s: head_dim %d not built (64, 128, 192)", who, D);
    MI355_REQUIRE(R >= 2 && R <= D && R % 2 == 0, "%s: rotated width %d must be even and in [2, head_dim = %d]", who, R, D);
    MI355_REQUIRE(ldx >= (int64_t)(Hq + Hkv) * D && ldy >= (int64_t)(Hq + Hkv) * D, "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(table_rows >= S, "%s: coefficient table has %lld rows, sequence length is %d", who, (long long)table_rows, S);
    return 0;
}

inline int row_grid(int64_t rows) {
    int64_t g = (rows + 3) / 4;
    return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" int mi355_sink_attn_fwd(int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, const float* sink, void* o, int64_t ldo, float* lse, float scale, void* stream) {
    if (check_sink("mi355_sink_attn_fwd", B, S, Hq, Hkv, D, DV, W, ldq, ldk, ldv, ldo)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(q && k && v && o && lse, "mi355_sink_attn_fwd: null pointer");
    MI355_REQUIRE(aligned16({q, k, v, o}), "mi355_sink_attn_fwd: q, k, v, o must be 16-byte aligned");
    const int w = W < S ? W : S;
    dim3 grid((S + 127) / 128, Hq, B);
#define X(DD, VV)                                                                                                                                        \
    if (D == DD && DV == VV)                                                                                                                             \
        sink_fwd_kernel<DD, VV><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, sink,  \
                                                              (bf16_t*)o, ldo, lse, scale * LOG2E);
    MIMO_PAIRS(X)
#undef X
    MI355_LAUNCH_CHECK("mi355_sink_attn_fwd");
    return 0;
}

extern "C" int mi355_sink_attn_bwd(int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo, const float* sink,
                                   const float* lse, float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                   float* dsink_partial, int parts, float scale, void* stream) {
    if (check_sink("mi355_sink_attn_bwd", B, S, Hq, Hkv, D, DV, W, ldq, ldk, ldv, ldo)) return 1;
    if (check_sink("mi355_sink_attn_bwd", B, S, Hq, Hkv, D, DV, W, lddq, lddk, lddv, lddo)) return 1;
    MI355_REQUIRE(!sink || (dsink_partial && parts >= 1 && parts <= 65535),
                  "mi355_sink_attn_bwd: with a sink, dsink_partial must be given and parts in 1..65535 (got %d)", parts);
    if (B == 0 || S == 0) return 0;  // an empty problem: nothing is written, dsink_partial included
    MI355_REQUIRE(q && k && v && o && d_o && lse && delta && dq && dk && dv, "mi355_sink_attn_bwd: null pointer");
    MI355_REQUIRE(aligned16({q, k, v, d_o, dq, dk, dv}), "mi355_sink_attn_bwd: q, k, v, d_o, dq, dk, dv must be 16-byte aligned");
    const int w = W < S ? W : S;
    const int64_t tokens = (int64_t)B * S;
    const int64_t dg = (tokens * Hq + 3) / 4;
    attn_delta_kernel<<<(int)(dg > 8192 ? 8192 : dg), 256, 0, ST(stream)>>>(tokens, S, Hq, DV, (const bf16_t*)o, ldo, (const bf16_t*)d_o, lddo, delta);
    MI355_LAUNCH_CHECK("mi355_sink_attn_bwd(delta)");
    if (sink) {
        sink_grad_kernel<<<parts, 256, 0, ST(stream)>>>(B, S, Hq, sink, lse, delta, dsink_partial);
        MI355_LAUNCH_CHECK("mi355_sink_attn_bwd(sink gradient)");
    }
    dim3 gq((S + 127) / 128, Hq, B), gk((S + 127) / 128, Hkv, B);
#define X(DD, VV)                                                                                                                                         \
    if (D == DD && DV == VV) {                                                                                                                            \
        sink_bwd_dq_kernel<DD, VV><<<gq, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv,        \
                                                               (const bf16_t*)d_o, lddo, lse, delta, (bf16_t*)dq, lddq, scale);                           \
        sink_bwd_dkv_kernel<DD, VV><<<gk, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv,       \
                                                                (const bf16_t*)d_o, lddo, lse, delta, (bf16_t*)dk, lddk, (bf16_t*)dv, lddv, scale);       \
    }
    MIMO_PAIRS(X)
#undef X
    MI355_LAUNCH_CHECK("mi355_sink_attn_bwd");
    return 0;
}

extern "C" int mi355_mimo_normrope_fwd(int64_t tokens, int S, int Hq, int Hkv, int D, int R, const void* x, int64_t ldx, const void* q_weight,
                                       const void* k_weight, const float* cos_t, const float* sin_t, int64_t table_rows, void* y, int64_t ldy,
                                       float eps, void* stream) {
    if (check_normrope("mi355_mimo_normrope_fwd", tokens, S, Hq, Hkv, D, R, ldx, ldy, table_rows)) return 1;
    if (tokens == 0) return 0;
    MI355_REQUIRE(x && q_weight && k_weight && cos_t && sin_t && y, "mi355_mimo_normrope_fwd: null pointer");
    const int grid = row_grid(tokens * (Hq + Hkv));
#define LAUNCH(DD)                                                                                                                                    \
    mimo_normrope_kernel<DD, false><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, Hkv, R, (const bf16_t*)x, ldx, (const bf16_t*)q_weight,                \
                                                                 (const bf16_t*)k_weight, cos_t, sin_t, nullptr, 0, (bf16_t*)y, ldy, nullptr, eps)
    switch (D) {
        case 64: LAUNCH(64); break;
        case 128: LAUNCH(128); break;
        default: LAUNCH(192); break;
    }
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_mimo_normrope_fwd");
    return 0;
}

extern "C" int mi355_mimo_normrope_bwd(int64_t tokens, int S, int Hq, int Hkv, int D, int R, const void* x, int64_t ldx, const void* q_weight,
                                       const void* k_weight, const float* cos_t, const float* sin_t, int64_t table_rows, const void* dy, int64_t lddy,
                                       void* dx, int64_t lddx, float* partial, int parts, float eps, void* stream) {
    if (check_normrope("mi355_mimo_normrope_bwd", tokens, S, Hq, Hkv, D, R, ldx, lddy, table_rows)) return 1;
    MI355_REQUIRE(lddx >= (int64_t)(Hq + Hkv) * D, "mi355_mimo_normrope_bwd: leading dimension smaller than heads*head_dim");
    MI355_REQUIRE(tokens > 0 && parts > 0 && parts <= 65535, "mi355_mimo_normrope_bwd: tokens must be positive and parts in 1..65535 (got %d)", parts);
    MI355_REQUIRE(x && q_weight && k_weight && cos_t && sin_t && dy && dx && partial, "mi355_mimo_normrope_bwd: null pointer");
#define LAUNCH(DD)                                                                                                                                    \
    mimo_normrope_kernel<DD, true><<<parts, 256, 0, ST(stream)>>>(tokens, S, Hq, Hkv, R, (const bf16_t*)x, ldx, (const bf16_t*)q_weight,                \
                                                                 (const bf16_t*)k_weight, cos_t, sin_t, (const bf16_t*)dy, lddy, (bf16_t*)dx, lddx,     \
                                                                 partial, eps)
    switch (D) {
        case 64: LAUNCH(64); break;
        case 128: LAUNCH(128); break;
        default: LAUNCH(192); break;
    }
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_mimo_normrope_bwd");
    return 0;
}
