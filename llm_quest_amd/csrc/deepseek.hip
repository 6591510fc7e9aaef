// DeepSeek-V3 (reference llama3_to_deepseekv3/): Multi-head Latent Attention core and the decoupled-RoPE row kernels.
//
// MLA causal attention (MultiLatentAttention.forward, deepseek_attention.py:78-106, where q and k are torch.cat'ed and the decoupled key is
// expand()ed to every head):
//   s(i, j) = scale * (q_nope_i . k_nope_j + q_rope_i . k_rope_j),  j <= i;  o_i = softmax_j(s) v_j
// The score contraction is DK = Dn + Dr wide, the value / context contraction Dn; k_rope is ONE Dr-wide row per token shared by all heads.
// Same data flow as attention_generic.hip / attention_band.hip -- S^T = K Q^T with the query on the MFMA lane (mfma_f32_32x32x16_bf16), lane-local online
// softmax in fp32, P^T packed from the accumulators as the B operand of O^T += V^T P^T, plain padded LDS images, one 32-key tile per barrier pair,
// no pipelining; backward with delta = rowsum(dO * O), a query-major dQ pass and a key-major dK/dV pass, no atomics.  What differs: the K image
// (32 x DK) is composed in LDS from two sources, the head's k_nope columns and the shared k_rope columns, the V image is Dn wide, nothing is
// padded and k_rope is never expanded in memory.  The gradient of the shared key is written per head into an fp32 scratch [T, Hq, Dr]; the RoPE
// backward below sums it over heads in a fixed order -- the one place where the "shared across heads" gradient is reduced.
// At (Dn, Dr) = (128, 64) the key-major pass holds dK^T (192 wide) and dV^T (128 wide): it runs as two slices (blockIdx.x = key_block * 2 + slice),
// each with 3 dK^T and 2 dV^T tiles, as the generic kernel does for d_h = 256.
//
// Decoupled RoPE (deepseek_attention.py:79-87): half-split rotation cos * x + sin * rotate_half(x) of the q_rope heads and of the shared key,
// position = token index inside its sequence, cos / sin rounded to bf16 first (the reference casts the tables to x.dtype), fp32 math, one rounding.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   kernel                          VGPR  AGPR  scratch  LDS bytes  waves/SIMD
//   mla_fwd_kernel<64, 32>           114    32        0      11264           3
//   mla_fwd_kernel<128, 64>          201    64        0      21504           1
//   mla_bwd_dq_kernel<64, 32>        130    48        0      11264           2
//   mla_bwd_dq_kernel<128, 64>       235    96        0      21504           1
//   mla_bwd_dkv_kernel<64, 32, 1>    204    80        0      11520           1
//   mla_bwd_dkv_kernel<128, 64, 2>   252    80        0      21760           1
//   mla_rope_kernel<32 | 64, fwd>     24     0        0          0           8
//   mla_rope_kernel<32 | 64, bwd>     22     0        0          0           8
//   attn_delta_kernel                 31     0        0          0           8
// LDS row pitches are 2 * D + 16 bytes: 208 (DK = 96) and 400 (DK = 192) put 16 consecutive rows' 16-byte fragments on 16 distinct 4-bank groups,
// as 144 / 272 do for the 64- / 128-wide V image, so the ds_read_b128 of frag_rows stays conflict-free; the ds_read_b64_tr_b16 of frag_cols reads
// the images exactly as the generic and sliding-window kernels do.
#include <initializer_list>

#include "host_checks.h"

#include "attn_tile32.h"
#include "rows_bf16.h"

namespace {

// columns [c0, c0 + DS) of a 32-row LDS image of pitch Tile32<DI>::PITCH, from rows base, base + ld, ..; rows >= rows_valid are zero
template <int DI, int DS, int NT>
__device__ __forceinline__ void load_tile_cols(char* img, int c0, const bf16_t* base, int64_t ld, int rows_valid, int tid) {
    constexpr int CH = DS / 8;
    for (int c = tid; c < 32 * CH; c += NT) {
        const int row = c / CH, ch = c % CH;
        u32x4 v = {0, 0, 0, 0};
        if (row < rows_valid) v = *reinterpret_cast<const u32x4*>(base + (int64_t)row * ld + ch * 8);
        *reinterpret_cast<u32x4*>(img + row * Tile32<DI>::PITCH + c0 * 2 + ch * 16) = v;
    }
}
// B operand fragments of the row cat(nope, rope) held on the lane
template <int DN, int DR>
__device__ __forceinline__ void load_cat_frags(const bf16_t* nope, const bf16_t* rope, bool valid, int lane, bf16x8 (&f)[(DN + DR) / 16]) {
#pragma unroll
    for (int ks = 0; ks < (DN + DR) / 16; ++ks) {
        u32x4 v = {0, 0, 0, 0};
        const bf16_t* src = ks < DN / 16 ? nope + 16 * ks : rope + 16 * (ks - DN / 16);
        if (valid) v = *reinterpret_cast<const u32x4*>(src + 8 * (lane >> 5));
        f[ks] = __builtin_bit_cast(bf16x8, v);
    }
}
// accumulator tile [32 d x 32 rows-on-lane] -> a token-major fp32 row (4 consecutive d per 16-byte store)
__device__ __forceinline__ void store_t_tile_f32(const f32x16& acc, float* rowptr, bool valid, int lane) {
    if (!valid) return;
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
        f32x4 w = {acc[4 * i4], acc[4 * i4 + 1], acc[4 * i4 + 2], acc[4 * i4 + 3]};
        *reinterpret_cast<f32x4*>(rowptr + 8 * i4 + 4 * (lane >> 5)) = w;
    }
}
__device__ __forceinline__ void store_t_tile_bf16(const f32x16& acc, float mul, bf16_t* rowptr, bool valid, int lane) {
    if (!valid) return;
#pragma unroll
    for (int i4 = 0; i4 < 4; ++i4) {
        u32x2 w;
        w[0] = pack_bf2(acc[4 * i4] * mul, acc[4 * i4 + 1] * mul);
        w[1] = pack_bf2(acc[4 * i4 + 2] * mul, acc[4 * i4 + 3] * mul);
        *reinterpret_cast<u32x2*>(rowptr + 8 * i4 + 4 * (lane >> 5)) = w;
    }
}

// ------------------------------------------------------------------------------------------------ MLA attention, forward
// S <= 2^30 (check_mla): every index sum below (qb + 127, key0 + 31, ..) stays inside int; token offsets are int64_t.
template <int DN, int DR>
__global__ __launch_bounds__(256) void mla_fwd_kernel(int S, int Hq, const bf16_t* __restrict__ qn, int64_t ldqn, const bf16_t* __restrict__ qr,
                                                      int64_t ldqr, const bf16_t* __restrict__ kn, int64_t ldkn, const bf16_t* __restrict__ kr,
                                                      int64_t ldkr, const bf16_t* __restrict__ v, int64_t ldv, bf16_t* __restrict__ o, int64_t ldo,
                                                      float* __restrict__ lse, float scale_log2) {
    constexpr int DK = DN + DR;
    using CK = Tile32<DK>;
    using CV = Tile32<DN>;
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    char* kimg = smem;
    char* vimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 qf[CK::KS];
    load_cat_frags<DN, DR>(qn + (tok0 + query) * ldqn + (int64_t)h * DN, qr + (tok0 + query) * ldqr + (int64_t)h * DR, qvalid, lane, qf);
    f32x16 acc[CV::DT];
    zero_tiles(acc);
    float m = NEG_INF, l = 0.f;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    for (int kt = 0; kt <= qlast / 32; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile_cols<DK, DN, 256>(kimg, 0, kn + (tok0 + key0) * ldkn + (int64_t)h * DN, ldkn, S - key0, threadIdx.x);
        load_tile_cols<DK, DR, 256>(kimg, DN, kr + (tok0 + key0) * ldkr, ldkr, S - key0, threadIdx.x);
        load_tile<DN, 256>(vimg, v + (tok0 + key0) * ldv + (int64_t)h * DN, ldv, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31) continue;  // tile above this wave's diagonal
        f32x16 s;
        zero_tile(s);
        mma_rows<DK>(s, kimg, qf, lane);
        float mx = NEG_INF;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = key < S && key <= query;
            s[i] = ok ? s[i] * scale_log2 : NEG_INF;
            mx = fmaxf(mx, s[i]);
        }
        online_softmax(s, mx, m, l, acc);
        const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CV::DT; ++dt) mma_cols<DN>(acc[dt], vimg, 32 * dt, p0, p1, lane);
    }
    store_t_tiles<CV::DT>(acc, 1.f / l, o + (tok0 + query) * ldo + (int64_t)h * DN, qvalid, lane);
    if (lane < 32 && qvalid) lse[((int64_t)b * Hq + h) * S + query] = (m + log2f(l)) * LN2;
}

// ------------------------------------------------------------------------------------------------ dQ pass (query-major)
template <int DN, int DR>
__global__ __launch_bounds__(256) void mla_bwd_dq_kernel(int S, int Hq, const bf16_t* __restrict__ qn, int64_t ldqn, const bf16_t* __restrict__ qr,
                                                         int64_t ldqr, const bf16_t* __restrict__ kn, int64_t ldkn, const bf16_t* __restrict__ kr,
                                                         int64_t ldkr, const bf16_t* __restrict__ v, int64_t ldv, const bf16_t* __restrict__ d_o,
                                                         int64_t lddo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                         bf16_t* __restrict__ dqn, int64_t lddqn, bf16_t* __restrict__ dqr, int64_t lddqr, float scale) {
    constexpr int DK = DN + DR;
    using CK = Tile32<DK>;
    using CV = Tile32<DN>;
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    char* kimg = smem;
    char* vimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const int query = q0 + (lane & 31);
    const bool qvalid = query < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 qf[CK::KS], gf[CV::KS];
    load_cat_frags<DN, DR>(qn + (tok0 + query) * ldqn + (int64_t)h * DN, qr + (tok0 + query) * ldqr + (int64_t)h * DR, qvalid, lane, qf);
    load_row_frags<DN>(d_o + (tok0 + query) * lddo + (int64_t)h * DN, qvalid, lane, gf);
    const float lse_q = qvalid ? lse[((int64_t)b * Hq + h) * S + query] * LOG2E : 0.f;
    const float delta_q = qvalid ? delta[((int64_t)b * Hq + h) * S + query] : 0.f;
    const float scale_log2 = scale * LOG2E;
    f32x16 acc[CK::DT];
    zero_tiles(acc);
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    for (int kt = 0; kt <= qlast / 32; ++kt) {
        const int key0 = kt * 32;
        __syncthreads();
        load_tile_cols<DK, DN, 256>(kimg, 0, kn + (tok0 + key0) * ldkn + (int64_t)h * DN, ldkn, S - key0, threadIdx.x);
        load_tile_cols<DK, DR, 256>(kimg, DN, kr + (tok0 + key0) * ldkr, ldkr, S - key0, threadIdx.x);
        load_tile<DN, 256>(vimg, v + (tok0 + key0) * ldv + (int64_t)h * DN, ldv, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31) continue;
        f32x16 s, dp;
        zero_tile(s);
        zero_tile(dp);
        mma_rows<DK>(s, kimg, qf, lane);
        mma_rows<DN>(dp, vimg, gf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = key0 + acc_row(i, lane);
            const bool ok = qvalid && key <= query;
            const float p = ok ? exp2f(s[i] * scale_log2 - lse_q) : 0.f;
            s[i] = p * (dp[i] - delta_q) * scale;
        }
        const bf16x8 d0 = pack_frag(s, 0), d1 = pack_frag(s, 1);
#pragma unroll
        for (int dt = 0; dt < CK::DT; ++dt) mma_cols<DK>(acc[dt], kimg, 32 * dt, d0, d1, lane);
    }
    bf16_t* on = dqn + (tok0 + query) * lddqn + (int64_t)h * DN;
    bf16_t* orp = dqr + (tok0 + query) * lddqr + (int64_t)h * DR;
#pragma unroll
    for (int dt = 0; dt < CK::DT; ++dt) store_t_tile_bf16(acc[dt], 1.f, dt < CV::DT ? on + 32 * dt : orp + 32 * (dt - CV::DT), qvalid, lane);
}

// ------------------------------------------------------------------------------------------------ dK/dV pass (key-major)
// A wave owns 32 keys of one head and walks the query tiles from the diagonal on.  NP = number of slices the dK^T (DK wide) and dV^T (DN wide)
// accumulators are split into (blockIdx.x = key_block * NP + slice); dK^T tiles at columns >= DN are the head's share of the shared key's
// gradient and go to the fp32 scratch dkr_heads [T, Hq, DR].
template <int DN, int DR, int NP>
__global__ __launch_bounds__(256) void mla_bwd_dkv_kernel(int S, int Hq, const bf16_t* __restrict__ qn, int64_t ldqn, const bf16_t* __restrict__ qr,
                                                          int64_t ldqr, const bf16_t* __restrict__ kn, int64_t ldkn, const bf16_t* __restrict__ kr,
                                                          int64_t ldkr, const bf16_t* __restrict__ v, int64_t ldv, const bf16_t* __restrict__ d_o,
                                                          int64_t lddo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                          bf16_t* __restrict__ dkn, int64_t lddkn, float* __restrict__ dkr_heads,
                                                          bf16_t* __restrict__ dv, int64_t lddv, float scale) {
    constexpr int DK = DN + DR;
    using CK = Tile32<DK>;
    using CV = Tile32<DN>;
    constexpr int NK = CK::DT / NP, NV = CV::DT / NP;
    static_assert(NK * NP == CK::DT && NV * NP == CV::DT, "the slices must divide both accumulators");
    __shared__ __attribute__((aligned(16))) char smem[CK::IMG + CV::IMG];
    __shared__ float stat[2][32];
    char* qimg = smem;
    char* gimg = smem + CK::IMG;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int kb = (blockIdx.x / NP) * 128, slice = blockIdx.x % NP;
    const int k0 = kb + wave * 32;
    const int key = k0 + (lane & 31);
    const bool kvalid = key < S;
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 kf[CK::KS], vf[CV::KS];
    load_cat_frags<DN, DR>(kn + (tok0 + key) * ldkn + (int64_t)h * DN, kr + (tok0 + key) * ldkr, kvalid, lane, kf);
    load_row_frags<DN>(v + (tok0 + key) * ldv + (int64_t)h * DN, kvalid, lane, vf);
    const float scale_log2 = scale * LOG2E;
    f32x16 adk[NK], adv[NV];
    zero_tiles(adk);
    zero_tiles(adv);
    for (int qt = kb / 32; qt <= (S - 1) / 32; ++qt) {
        const int qs = qt * 32;
        __syncthreads();
        load_tile_cols<DK, DN, 256>(qimg, 0, qn + (tok0 + qs) * ldqn + (int64_t)h * DN, ldqn, S - qs, threadIdx.x);
        load_tile_cols<DK, DR, 256>(qimg, DN, qr + (tok0 + qs) * ldqr + (int64_t)h * DR, ldqr, S - qs, threadIdx.x);
        load_tile<DN, 256>(gimg, d_o + (tok0 + qs) * lddo + (int64_t)h * DN, lddo, S - qs, threadIdx.x);
        if (threadIdx.x < 32) {
            const bool okq = qs + threadIdx.x < S;
            stat[0][threadIdx.x] = okq ? lse[((int64_t)b * Hq + h) * S + qs + threadIdx.x] * LOG2E : 0.f;
            stat[1][threadIdx.x] = okq ? delta[((int64_t)b * Hq + h) * S + qs + threadIdx.x] : 0.f;
        }
        __syncthreads();
        if (k0 >= S || qs + 31 < k0) continue;  // every query of the tile precedes this wave's keys
        f32x16 s, dp;
        zero_tile(s);
        zero_tile(dp);
        mma_rows<DK>(s, qimg, kf, lane);
        mma_rows<DN>(dp, gimg, vf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = acc_row(i, lane);
            const int qi = qs + r;
            const bool ok = kvalid && qi < S && key <= qi;
            const float p = ok ? exp2f(s[i] * scale_log2 - stat[0][r]) : 0.f;
            s[i] = p;
            dp[i] = p * (dp[i] - stat[1][r]) * scale;
        }
        const bf16x8 p0 = pack_frag(s, 0), p1 = pack_frag(s, 1), d0 = pack_frag(dp, 0), d1 = pack_frag(dp, 1);
#pragma unroll
        for (int dt = 0; dt < NV; ++dt) {
            const int c0 = 32 * (slice * NV + dt);
            mma_cols<DN>(adv[dt], gimg, c0, p0, p1, lane);
        }
#pragma unroll
        for (int dt = 0; dt < NK; ++dt) {
            const int c0 = 32 * (slice * NK + dt);
            mma_cols<DK>(adk[dt], qimg, c0, d0, d1, lane);
        }
    }
    bf16_t* okn = dkn + (tok0 + key) * lddkn + (int64_t)h * DN;
    float* okr = dkr_heads + ((tok0 + key) * Hq + h) * DR;
#pragma unroll
    for (int dt = 0; dt < NK; ++dt) {
        const int c0 = 32 * (slice * NK + dt);  // a 32-column tile lies wholly on one side of DN (a multiple of 32)
        if (c0 < DN)
            store_t_tile_bf16(adk[dt], 1.f, okn + c0, kvalid, lane);
        else
            store_t_tile_f32(adk[dt], okr + (c0 - DN), kvalid, lane);
    }
    bf16_t* ov = dv + (tok0 + key) * lddv + (int64_t)h * DN + 32 * slice * NV;
#pragma unroll
    for (int dt = 0; dt < NV; ++dt) store_t_tile_bf16(adv[dt], 1.f, ov + 32 * dt, kvalid, lane);
}

// ------------------------------------------------------------------------------------------------ decoupled RoPE
// A row is one (token, head): head < Hq a q_rope head, head == Hq the token's shared key.  A lane owns feature j of the first half and its partner
// j + DR/2, so a wave covers 128 / DR rows at a time.  BWD: the adjoint rotation; the key row first sums the per-head fp32 scratch over heads
// 0, 1, .., Hq - 1 in that order.
template <int DR, bool BWD>
__global__ __launch_bounds__(256) void mla_rope_kernel(int64_t tokens, int S, int Hq, const bf16_t* __restrict__ xq, int64_t ldxq,
                                                       const bf16_t* __restrict__ xk, int64_t ldxk, const float* __restrict__ xk_heads,
                                                       const float* __restrict__ cos_t, const float* __restrict__ sin_t, bf16_t* __restrict__ yq,
                                                       int64_t ldyq, bf16_t* __restrict__ yk, int64_t ldyk) {
    constexpr int HALF = DR / 2, RPW = 64 / HALF;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / HALF, j = lane % HALF;
    const int H = Hq + 1;
    const int64_t total = tokens * H;
    const int64_t groups = (total + RPW - 1) / RPW;
    for (int64_t g = (int64_t)blockIdx.x * 4 + wv; g < groups; g += (int64_t)gridDim.x * 4) {
        const int64_t row = g * RPW + sub;
        if (row >= total) continue;
        const int64_t t = row / H;
        const int h = (int)(row % H);
        const int pos = (int)(t % S);
        float x1, x2;
        if (h < Hq) {
            x1 = bf2f(xq[t * ldxq + (int64_t)h * DR + j]);
            x2 = bf2f(xq[t * ldxq + (int64_t)h * DR + j + HALF]);
        } else if (!BWD) {
            x1 = bf2f(xk[t * ldxk + j]);
            x2 = bf2f(xk[t * ldxk + j + HALF]);
        } else {
            x1 = x2 = 0.f;
            for (int hh = 0; hh < Hq; ++hh) {
                x1 += xk_heads[(t * Hq + hh) * DR + j];
                x2 += xk_heads[(t * Hq + hh) * DR + j + HALF];
            }
        }
        const float c1 = rbf(cos_t[(int64_t)pos * DR + j]), c2 = rbf(cos_t[(int64_t)pos * DR + j + HALF]);
        const float s1 = rbf(sin_t[(int64_t)pos * DR + j]), s2 = rbf(sin_t[(int64_t)pos * DR + j + HALF]);
        // forward: cos * x + sin * cat(-x2, x1);  backward: cos * g + (z2, -z1), z = sin * g
        const float r1 = BWD ? c1 * x1 + s2 * x2 : c1 * x1 - s1 * x2;
        const float r2 = BWD ? c2 * x2 - s1 * x1 : c2 * x2 + s2 * x1;
        bf16_t* y = h < Hq ? yq + t * ldyq + (int64_t)h * DR : yk + t * ldyk;
        y[j] = f2bf(r1);
        y[j + HALF] = f2bf(r2);
    }
}

bool lds_ok(std::initializer_list<int64_t> lds, int64_t least) {
    for (int64_t ld : lds)
        if (ld < least || ld % 8) return false;
    return true;
}

int check_mla(const char* who, int B, int S, int Hq, int Dn, int Dr) {
    MI355_REQUIRE(B > 0 && S > 0 && Hq > 0, "%s: batch (%d), sequence length (%d) and heads (%d) must be positive", who, B, S, Hq);
    MI355_REQUIRE((Dn == 64 && Dr == 32) || (Dn == 128 && Dr == 64), "%s: (head_dim, rope_dim) = (%d, %d) not built: (64, 32) and (128, 64)", who, Dn, Dr);
    // S <= 2^30: the largest int expression in the kernels is a tile start plus 127 + 32, below S + 160; the grid's x is at most 2 * (S / 128 + 1)
    MI355_REQUIRE(B <= 65535 && Hq <= 65535 && S <= (1 << 30), "%s: grid limits (B, Hq <= 65535, S <= 2^30)", who);
    return 0;
}

// Not host_checks.h's row_grid: this one counts groups of 128 / Dr rows (what a wave of mla_rope_kernel covers per trip) and caps the grid at 4096
// workgroups where row_grid caps at 2048.  Merging the two would change the launch grids of mi355_mla_rope_*.
inline int group_grid(int64_t groups) {
    int64_t g = (groups + 3) / 4;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

int check_mla_rope(const char* who, int64_t tokens, int S, int Hq, int Dr, int64_t table_rows) {
    MI355_REQUIRE(tokens > 0 && S > 0 && Hq > 0 && tokens % S == 0, "%s: tokens (%lld) must be a positive multiple of the sequence length (%d), heads (%d) positive",
                  who, (long long)tokens, S, Hq);
    MI355_REQUIRE(Dr == 32 || Dr == 64, "%s: rope_dim %d not built (32, 64)", who, Dr);
    MI355_REQUIRE(Hq <= 65535, "%s: at most 65535 heads", who);
    MI355_REQUIRE(table_rows >= S, "%s: coefficient table has %lld rows, sequence length is %d", who, (long long)table_rows, S);
    return 0;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))
#define BF(p) ((const bf16_t*)(p))

extern "C" int mi355_mla_attn_fwd(int B, int S, int Hq, int Dn, int Dr, const void* q_nope, int64_t ldqn, const void* q_rope, int64_t ldqr,
                                  const void* k_nope, int64_t ldkn, const void* k_rope, int64_t ldkr, const void* v, int64_t ldv, void* o, int64_t ldo,
                                  float* lse, float scale, void* stream) {
    if (check_mla("mi355_mla_attn_fwd", B, S, Hq, Dn, Dr)) return 1;
    MI355_REQUIRE(lds_ok({ldqn, ldkn, ldv, ldo}, (int64_t)Hq * Dn) && lds_ok({ldqr}, (int64_t)Hq * Dr) && lds_ok({ldkr}, Dr),
                  "mi355_mla_attn_fwd: a leading dimension is smaller than its row (Hq*Dn, Hq*Dr, Dr) or no multiple of 8");
    MI355_REQUIRE(q_nope && q_rope && k_nope && k_rope && v && o && lse, "mi355_mla_attn_fwd: null pointer");
    MI355_REQUIRE(aligned16({q_nope, q_rope, k_nope, k_rope, v, o}), "mi355_mla_attn_fwd: operands must be 16-byte aligned");
    dim3 grid((S + 127) / 128, Hq, B);
#define LAUNCH(DN_, DR_)                                                                                                                              \
    mla_fwd_kernel<DN_, DR_><<<grid, 256, 0, ST(stream)>>>(S, Hq, BF(q_nope), ldqn, BF(q_rope), ldqr, BF(k_nope), ldkn, BF(k_rope), ldkr, BF(v), ldv, \
                                                           (bf16_t*)o, ldo, lse, scale * LOG2E)
    if (Dn == 64)
        LAUNCH(64, 32);
    else
        LAUNCH(128, 64);
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_mla_attn_fwd");
    return 0;
}

extern "C" int mi355_mla_attn_bwd(int B, int S, int Hq, int Dn, int Dr, const void* q_nope, int64_t ldqn, const void* q_rope, int64_t ldqr,
                                  const void* k_nope, int64_t ldkn, const void* k_rope, int64_t ldkr, const void* v, int64_t ldv, const void* o,
                                  int64_t ldo, const void* d_o, int64_t lddo, const float* lse, float* delta, void* dq_nope, int64_t lddqn,
                                  void* dq_rope, int64_t lddqr, void* dk_nope, int64_t lddkn, float* dk_rope_heads, void* dv, int64_t lddv, float scale,
                                  void* stream) {
    if (check_mla("mi355_mla_attn_bwd", B, S, Hq, Dn, Dr)) return 1;
    MI355_REQUIRE(lds_ok({ldqn, ldkn, ldv, ldo, lddo, lddqn, lddkn, lddv}, (int64_t)Hq * Dn) && lds_ok({ldqr, lddqr}, (int64_t)Hq * Dr) && lds_ok({ldkr}, Dr),
                  "mi355_mla_attn_bwd: a leading dimension is smaller than its row (Hq*Dn, Hq*Dr, Dr) or no multiple of 8");
    MI355_REQUIRE(q_nope && q_rope && k_nope && k_rope && v && o && d_o && lse && delta && dq_nope && dq_rope && dk_nope && dk_rope_heads && dv,
                  "mi355_mla_attn_bwd: null pointer");
    MI355_REQUIRE(aligned16({q_nope, q_rope, k_nope, k_rope, v, d_o, dq_nope, dq_rope, dk_nope, dk_rope_heads, dv}),
                  "mi355_mla_attn_bwd: operands must be 16-byte aligned");
    const int64_t tokens = (int64_t)B * S;
    const int64_t dg = (tokens * Hq + 3) / 4;
    attn_delta_kernel<<<(int)(dg > 8192 ? 8192 : dg), 256, 0, ST(stream)>>>(tokens, S, Hq, Dn, BF(o), ldo, BF(d_o), lddo, delta);
    MI355_LAUNCH_CHECK("mi355_mla_attn_bwd(delta)");
    const int nb = (S + 127) / 128;
#define LAUNCH(DN_, DR_, NP_)                                                                                                                          \
    mla_bwd_dq_kernel<DN_, DR_><<<dim3(nb, Hq, B), 256, 0, ST(stream)>>>(S, Hq, BF(q_nope), ldqn, BF(q_rope), ldqr, BF(k_nope), ldkn, BF(k_rope), ldkr,  \
                                                                         BF(v), ldv, BF(d_o), lddo, lse, delta, (bf16_t*)dq_nope, lddqn,               \
                                                                         (bf16_t*)dq_rope, lddqr, scale);                                              \
    mla_bwd_dkv_kernel<DN_, DR_, NP_><<<dim3(nb * NP_, Hq, B), 256, 0, ST(stream)>>>(S, Hq, BF(q_nope), ldqn, BF(q_rope), ldqr, BF(k_nope), ldkn,       \
                                                                                     BF(k_rope), ldkr, BF(v), ldv, BF(d_o), lddo, lse, delta,          \
                                                                                     (bf16_t*)dk_nope, lddkn, dk_rope_heads, (bf16_t*)dv, lddv, scale)
    if (Dn == 64) {
        LAUNCH(64, 32, 1);
    } else {
        LAUNCH(128, 64, 2);
    }
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_mla_attn_bwd");
    return 0;
}

extern "C" int mi355_mla_rope_fwd(int64_t tokens, int S, int Hq, int Dr, const void* q_rope_pre, int64_t ldq, const void* k_rope_pre, int64_t ldk,
                                  const float* cos_t, const float* sin_t, int64_t table_rows, void* q_rope, int64_t ldqo, void* k_rope, int64_t ldko,
                                  void* stream) {
    if (check_mla_rope("mi355_mla_rope_fwd", tokens, S, Hq, Dr, table_rows)) return 1;
    MI355_REQUIRE(ldq >= (int64_t)Hq * Dr && ldqo >= (int64_t)Hq * Dr && ldk >= Dr && ldko >= Dr,
                  "mi355_mla_rope_fwd: a leading dimension is smaller than its row (Hq*Dr, Dr)");
    MI355_REQUIRE(q_rope_pre && k_rope_pre && cos_t && sin_t && q_rope && k_rope, "mi355_mla_rope_fwd: null pointer");
    const int grid = group_grid(tokens * (Hq + 1) / (128 / Dr) + 1);
    if (Dr == 32)
        mla_rope_kernel<32, false><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, BF(q_rope_pre), ldq, BF(k_rope_pre), ldk, nullptr, cos_t, sin_t,
                                                                 (bf16_t*)q_rope, ldqo, (bf16_t*)k_rope, ldko);
    else
        mla_rope_kernel<64, false><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, BF(q_rope_pre), ldq, BF(k_rope_pre), ldk, nullptr, cos_t, sin_t,
                                                                 (bf16_t*)q_rope, ldqo, (bf16_t*)k_rope, ldko);
    MI355_LAUNCH_CHECK("mi355_mla_rope_fwd");
    return 0;
}

extern "C" int mi355_mla_rope_bwd(int64_t tokens, int S, int Hq, int Dr, const void* dq_rope, int64_t lddq, const float* dk_rope_heads,
                                  const float* cos_t, const float* sin_t, int64_t table_rows, void* dq_rope_pre, int64_t lddqp, void* dk_rope_pre,
                                  int64_t lddkp, void* stream) {
    if (check_mla_rope("mi355_mla_rope_bwd", tokens, S, Hq, Dr, table_rows)) return 1;
    MI355_REQUIRE(lddq >= (int64_t)Hq * Dr && lddqp >= (int64_t)Hq * Dr && lddkp >= Dr,
                  "mi355_mla_rope_bwd: a leading dimension is smaller than its row (Hq*Dr, Dr)");
    MI355_REQUIRE(dq_rope && dk_rope_heads && cos_t && sin_t && dq_rope_pre && dk_rope_pre, "mi355_mla_rope_bwd: null pointer");
    const int grid = group_grid(tokens * (Hq + 1) / (128 / Dr) + 1);
    if (Dr == 32)
        mla_rope_kernel<32, true><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, BF(dq_rope), lddq, nullptr, 0, dk_rope_heads, cos_t, sin_t,
                                                                (bf16_t*)dq_rope_pre, lddqp, (bf16_t*)dk_rope_pre, lddkp);
    else
        mla_rope_kernel<64, true><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, BF(dq_rope), lddq, nullptr, 0, dk_rope_heads, cos_t, sin_t,
                                                                (bf16_t*)dq_rope_pre, lddqp, (bf16_t*)dk_rope_pre, lddkp);
    MI355_LAUNCH_CHECK("mi355_mla_rope_bwd");
    return 0;
}
