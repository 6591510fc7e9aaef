// Banded causal attention: the one kernel family behind Gemma3's sliding windows (mi355_swa_attn_fwd / _bwd, reference llama3_to_gemma3/
// gemma3_attention.py:49-128, where it is a [b, h, s, w, d] gather of key / value windows) and MiMo-V2-Flash's attention with a learnable sink
// and decoupled q/k and v head dims (mi355_sink_attn_fwd / _bwd, reference xiaomi/mimo_v2_flash_attention.py:100-130, where it is a dense masked
// score matrix with one extra column per head).
//   allowed(i, j) = i - W < j <= i,  W >= 1 (W >= S: plain causal);  s_ij = scale * q_i . k_j over D features;
//   p_ij = exp(s_ij - m_i) / (sum_j exp(s_ij - m_i) + exp(z_h - m_i));  o_i = sum_j p_ij v_j over DV features;  lse_i = log(sum_j exp(s_ij) + exp(z_h)).
// The sink logit z_h is NOT multiplied by the scale and has no value row; without a sink (NULL: always so for the windowed entry points, which also
// have DV = D) its two terms are absent.  The two ABI families are these same three kernels: one instantiation per (D, DV), here and nowhere else.
//
// Same data flow as attention_generic.hip -- S^T = K Q^T with the query on the MFMA lane (mfma_f32_32x32x16_bf16), lane-local online softmax,
// P^T packed from the accumulators as the B operand of O^T += V^T P^T, plain padded LDS images (the k image and the v image with their own widths),
// one 32-key tile per barrier pair, no pipelining; backward with delta = rowsum(dO * O), a query-major dQ pass and a key-major dK/dV pass, no
// atomics -- and one difference, which is the point: only the key tiles that meet the band are walked.  A workgroup of 128 queries starting at qb
// visits keys max(0, qb - W + 1) .. q_last; a workgroup of 128 keys [kb, k_last] visits queries kb .. min(S - 1, k_last + W - 1); inside it a wave
// skips the tiles outside its own 32 rows' band.  No row is ever fully masked (j = i is always allowed).  The host clamps W to S, so every W >= S
// runs the same instructions on the same numbers.
//
// The sink joins the online softmax as one more key without a value: the state (m, l, acc) of the tile loop is merged with (z_h log2(e), 1, 0)
// once, behind the loop.  In the backward delta_i = sum_d dO_i O_i is unchanged (the sink's value is zero) and p is recomputed from the saved lse,
// which already holds the sink.  Sink gradient: dz_h = - sum_{b,i} exp(z_h - lse[b,h,i]) delta[b,h,i], per-workgroup partial rows [parts, Hq] for
// mi355_reduce_rows_f32.
#include "attn_tile32.h"
#include "host_checks.h"

namespace {

// ------------------------------------------------------------------------------------------------ forward
// W is already clamped to [1, S] and S <= 2^30 - 64 (check_band): every sum of an index and W below stays inside int.
template <int D, int DV>
__global__ __launch_bounds__(256) void band_fwd_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
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
    zero_tiles(acc);
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
        zero_tile(s);
        mma_rows<D>(s, kimg, qf, lane);
        float mx = NEG_INF;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = key < S && key <= query && key + W > query;
            s[i] = ok ? s[i] * scale_log2 : NEG_INF;
            mx = fmaxf(mx, s[i]);
        }
        online_softmax(s, mx, m, l, acc);
        const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CV::DT; ++dt) mma_cols<DV>(acc[dt], vimg, 32 * dt, p0, p1, lane);
    }
    // the sink: one more "key" of logit z_h whose value row is zero, merged into the state (m, l, acc) like a last tile.  (Merged first, as the initial
    // state m = z_h log2 e, l = 1, the algebra is the same, but the compiler then holds the accumulators twice -- 62 AGPRs instead of 32 at (64, 64), a wave
    // per SIMD fewer -- and the forward is a third slower.)  A sink far below every score leaves m, l and the scale 1 / l exactly as they were; without
    // a sink the uniform branch is skipped and the write-out is the plain 1 / l.
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
__global__ __launch_bounds__(256) void band_bwd_dq_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
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
    zero_tiles(acc);
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
        zero_tile(s);
        zero_tile(dp);
        mma_rows<D>(s, kimg, qf, lane);
        mma_rows<DV>(dp, vimg, gf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = qvalid && key <= query && key + W > query;
            const float p = ok ? exp2f(s[i] * scale_log2 - lse_q) : 0.f;
            s[i] = p * (dp[i] - delta_q) * scale;
        }
        const bf16x8 d0 = pack_frag(s, 0), d1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CK::DT; ++dt) mma_cols<D>(acc[dt], kimg, 32 * dt, d0, d1, lane);
    }
    store_t_tiles<CK::DT>(acc, 1.f, dq + (tok0 + query) * lddq + (int64_t)h * D, qvalid, lane);
}

// ------------------------------------------------------------------------------------------------ dK/dV pass (key-major)
// A wave owns 32 keys of one kv head; all q heads of the group and the query tiles kb .. min(S - 1, k_last + W - 1) are walked.
template <int D, int DV>
__global__ __launch_bounds__(256) void band_bwd_dkv_kernel(int S, int Hq, int Hkv, int W, const bf16_t* __restrict__ q, int64_t ldq,
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
    zero_tiles(adk);
    zero_tiles(adv);
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
            zero_tile(s);
            zero_tile(dp);
            mma_rows<D>(s, qimg, kf, lane);
            mma_rows<DV>(dp, gimg, vf, lane);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = acc_row(i, lane);
                const int qi = qs + r;
                const bool ok = kvalid && qi < S && key <= qi && key + W > qi;
                const float p = ok ? exp2f(s[i] * scale_log2 - stat[0][r]) : 0.f;
                s[i] = p;
                dp[i] = p * (dp[i] - stat[1][r]) * scale;
            }
            const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1), d0 = pack_frag(dp, 0), d1 = pack_frag(dp, 1);
#pragma unroll
            for (int dt = 0; dt < CV::DT; ++dt) mma_cols<DV>(adv[dt], gimg, 32 * dt, p0, p1, lane);
#pragma unroll
            for (int dt = 0; dt < CK::DT; ++dt) mma_cols<D>(adk[dt], qimg, 32 * dt, d0, d1, lane);
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

// ------------------------------------------------------------------------------------------------ host side
// The sink entry points take the five pairs; the windowed ones take D = DV in {32, 64, 128}, of which (32, 32) is built for them alone.
// (192, 128) is the released MiMo model's pair: its three kernels need no scratch (dK/dV: 212 VGPRs + 192 AGPRs at one wave per SIMD).
#define SINK_PAIRS(X) X(64, 32) X(64, 64) X(128, 64) X(128, 128) X(192, 128)
#define SINK_PAIR_NAMES "(64, 32), (64, 64), (128, 64), (128, 128), (192, 128)"
#define BAND_PAIRS(X) X(32, 32) SINK_PAIRS(X)

bool sink_pair_built(int D, int DV) {
#define X(DD, VV) \
    if (D == DD && DV == VV) return true;
    SINK_PAIRS(X)
#undef X
    return false;
}

// windowed: called for mi355_swa_attn_* (DV == D, the head dims of that family), else for mi355_sink_attn_* (its pairs)
int check_band(const char* who, bool windowed, int B, int S, int Hq, int Hkv, int D, int DV, int W, int64_t ldq, int64_t ldk, int64_t ldv,
               int64_t ldo) {
    MI355_REQUIRE(B >= 0 && S >= 0, "%s: negative batch or sequence length", who);
    MI355_REQUIRE(W >= 1, "%s: window %d must be at least 1", who, W);
    MI355_REQUIRE(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "%s: query heads (%d) must be a multiple of kv heads (%d)", who, Hq, Hkv);
    if (windowed)
        MI355_REQUIRE(D == 32 || D == 64 || D == 128, "%s: head_dim %d not built (32, 64, 128)", who, D);
    else
        MI355_REQUIRE(sink_pair_built(D, DV), "%s: (head_dim, value_head_dim) = (%d, %d) not built " SINK_PAIR_NAMES, who, D, DV);
    MI355_REQUIRE(ldq >= (int64_t)Hq * D && ldo >= (int64_t)Hq * DV && ldk >= (int64_t)Hkv * D && ldv >= (int64_t)Hkv * DV,
                  "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0, "%s: leading dimensions must be multiples of 8 elements", who);
    // S <= 2^30 - 64: with W clamped to S the largest index sum in the kernels, k0 + 31 + W < 2 S + 32, stays inside int
    MI355_REQUIRE(B <= 65535 && Hq <= 65535 && S <= (1 << 30) - 64, "%s: grid limits (B, Hq <= 65535, S <= 2^30 - 64)", who);
    return 0;
}

int launch_failed(const char* who, const char* stage) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    mi355_set_error("%s%s: launch failed: %s", who, stage, hipGetErrorString(e));
    return 2;
}

#define ST(s) ((hipStream_t)(s))

int band_fwd(const char* who, bool windowed, int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k,
             int64_t ldk, const void* v, int64_t ldv, const float* sink, void* o, int64_t ldo, float* lse, float scale, void* stream) {
    if (check_band(who, windowed, B, S, Hq, Hkv, D, DV, W, ldq, ldk, ldv, ldo)) return 1;
    if (B == 0 || S == 0) return 0;
    MI355_REQUIRE(q && k && v && o && lse, "%s: null pointer", who);
    MI355_REQUIRE(aligned16({q, k, v, o}), "%s: q, k, v, o must be 16-byte aligned", who);
    const int w = W < S ? W : S;
    dim3 grid((S + 127) / 128, Hq, B);
#define X(DD, VV)                                                                                                                                        \
    if (D == DD && DV == VV)                                                                                                                             \
        band_fwd_kernel<DD, VV><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, sink,  \
                                                              (bf16_t*)o, ldo, lse, scale * LOG2E);
    BAND_PAIRS(X)
#undef X
    return launch_failed(who, "");
}

// dsink_partial / parts: read with a sink only
int band_bwd(const char* who, bool windowed, int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k,
             int64_t ldk, const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo, const float* sink, const float* lse,
             float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, float* dsink_partial, int parts, float scale,
             void* stream) {
    if (check_band(who, windowed, B, S, Hq, Hkv, D, DV, W, ldq, ldk, ldv, ldo)) return 1;
    if (check_band(who, windowed, B, S, Hq, Hkv, D, DV, W, lddq, lddk, lddv, lddo)) return 1;
    MI355_REQUIRE(!sink || (dsink_partial && parts >= 1 && parts <= 65535),
                  "%s: with a sink, dsink_partial must be given and parts in 1..65535 (got %d)", who, parts);
    if (B == 0 || S == 0) return 0;  // an empty problem: nothing is written, dsink_partial included
    MI355_REQUIRE(q && k && v && o && d_o && lse && delta && dq && dk && dv, "%s: null pointer", who);
    MI355_REQUIRE(aligned16({q, k, v, d_o, dq, dk, dv}), "%s: q, k, v, d_o, dq, dk, dv must be 16-byte aligned", who);
    const int w = W < S ? W : S;
    const int64_t tokens = (int64_t)B * S;
    const int64_t dg = (tokens * Hq + 3) / 4;
    attn_delta_kernel<<<(int)(dg > 8192 ? 8192 : dg), 256, 0, ST(stream)>>>(tokens, S, Hq, DV, (const bf16_t*)o, ldo, (const bf16_t*)d_o, lddo, delta);
    if (int rc = launch_failed(who, "(delta)")) return rc;
    if (sink) {
        sink_grad_kernel<<<parts, 256, 0, ST(stream)>>>(B, S, Hq, sink, lse, delta, dsink_partial);
        if (int rc = launch_failed(who, "(sink gradient)")) return rc;
    }
    dim3 gq((S + 127) / 128, Hq, B), gk((S + 127) / 128, Hkv, B);
#define X(DD, VV)                                                                                                                                         \
    if (D == DD && DV == VV) {                                                                                                                            \
        band_bwd_dq_kernel<DD, VV><<<gq, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv,        \
                                                               (const bf16_t*)d_o, lddo, lse, delta, (bf16_t*)dq, lddq, scale);                           \
        band_bwd_dkv_kernel<DD, VV><<<gk, 256, 0, ST(stream)>>>(S, Hq, Hkv, w, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv,       \
                                                                (const bf16_t*)d_o, lddo, lse, delta, (bf16_t*)dk, lddk, (bf16_t*)dv, lddv, scale);       \
    }
    BAND_PAIRS(X)
#undef X
    return launch_failed(who, "");
}

}  // namespace

extern "C" int mi355_swa_attn_fwd(int B, int S, int Hq, int Hkv, int D, int W, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                  int64_t ldv, void* o, int64_t ldo, float* lse, float scale, void* stream) {
    return band_fwd("mi355_swa_attn_fwd", true, B, S, Hq, Hkv, D, D, W, q, ldq, k, ldk, v, ldv, nullptr, o, ldo, lse, scale, stream);
}

extern "C" int mi355_swa_attn_bwd(int B, int S, int Hq, int Hkv, int D, int W, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                  int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo, const float* lse, float* delta, void* dq,
                                  int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, float scale, void* stream) {
    return band_bwd("mi355_swa_attn_bwd", true, B, S, Hq, Hkv, D, D, W, q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, nullptr, lse, delta, dq, lddq, dk,
                    lddk, dv, lddv, nullptr, 0, scale, stream);
}

extern "C" int mi355_sink_attn_fwd(int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, const float* sink, void* o, int64_t ldo, float* lse, float scale, void* stream) {
    return band_fwd("mi355_sink_attn_fwd", false, B, S, Hq, Hkv, D, DV, W, q, ldq, k, ldk, v, ldv, sink, o, ldo, lse, scale, stream);
}

extern "C" int mi355_sink_attn_bwd(int B, int S, int Hq, int Hkv, int D, int DV, int W, const void* q, int64_t ldq, const void* k, int64_t ldk,
                                   const void* v, int64_t ldv, const void* o, int64_t ldo, const void* d_o, int64_t lddo, const float* sink,
                                   const float* lse, float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                                   float* dsink_partial, int parts, float scale, void* stream) {
    return band_bwd("mi355_sink_attn_bwd", false, B, S, Hq, Hkv, D, DV, W, q, ldq, k, ldk, v, ldv, o, ldo, d_o, lddo, sink, lse, delta, dq, lddq, dk,
                    lddk, dv, lddv, dsink_partial, parts, scale, stream);
}
