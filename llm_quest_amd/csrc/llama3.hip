// Llama 3.2 (reference gpt_to_llama3/) and QK-Clip (reference common/qk_clip.py): the three kernels the family needs beside what exists.
//
// Fused RoPE on the packed projection (llama_attention.py:78-79): qkv [M, (Hq + 2 Hkv) D] -> q [M, Hq D], k [M, Hkv D] in one launch, and the adjoint
//   rotation of dq, dk written into the q | k columns of d(qkv).  The arithmetic is that of rope_dropout.hip's bf16 path, rounding for rounding
//   (cos / sin rounded to bf16, each product and the sum rounded to bf16): the two agree bit for bit.
// Per-head maximum attention logit: out[h] = max over b and the visible (i, j) of scale * <q[b,i,h,:], k[b,j,h / (Hq / Hkv),:]>, visible = j <= i and
//   key_mask[b,j] != 0 -- the pairs the softmax of mi355_attn_fwd sees.  The first half of attention_band.hip's forward and nothing else: S^T = K Q^T with the
//   query on the MFMA lane (mfma_f32_32x32x16_bf16, fp32 accumulation), one plain padded LDS image of 32 keys per barrier pair, only the key tiles up to
//   the workgroup's diagonal.  No exp, no second product, no value tile; a workgroup of 128 queries leaves ONE float, and a second kernel folds the
//   B * ceil(S / 128) partials of each head.  No atomics.  A NaN among the visible logits of a head makes its result NaN (torch.amax); a head without a
//   visible pair yields -inf.
// QK-Clip: w = bf16(float(w) * s) on the D x d_in row block of every head that clips; gamma is computed on the device from the [Hq] maxima, a workgroup
//   whose head does not clip returns before it touches memory.
#include "host_checks.h"

#include "attn_tile32.h"

namespace {

// ------------------------------------------------------------------------------------------------ fused RoPE
__device__ __forceinline__ float rnd_bf(float v) { return bf2f(f2bf(v)); }

// One thread = 8 consecutive features of a head's first half and their partners in the second half.  BWD: x = (dq | dk), out = the q | k columns of dqkv.
template <int D, bool BWD>
__global__ __launch_bounds__(256) void llama_rope_kernel(int64_t tokens, int Hq, int Hkv, const bf16_t* __restrict__ xq, int64_t ldxq,
                                                         const bf16_t* __restrict__ xk, int64_t ldxk, const float* __restrict__ cosr,
                                                         const float* __restrict__ sinr, int64_t table_rows, const int32_t* __restrict__ pos,
                                                         bf16_t* __restrict__ oq, int64_t ldoq, bf16_t* __restrict__ ok, int64_t ldok) {
    constexpr int HALF = D / 2, CPH = HALF / 8;  // chunks per head
    const int H = Hq + Hkv;
    const int64_t total = tokens * H * CPH;
    for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < total; item += (int64_t)gridDim.x * 256) {
        const int c = (int)(item % CPH);
        const int h = (int)((item / CPH) % H);
        const int64_t t = item / ((int64_t)CPH * H);
        const bool isq = h < Hq;
        const bf16_t* xr = isq ? xq + t * ldxq + (int64_t)h * D : xk + t * ldxk + (int64_t)(h - Hq) * D;
        bf16_t* orow = isq ? oq + t * ldoq + (int64_t)h * D : ok + t * ldok + (int64_t)(h - Hq) * D;
        const int j = c * 8;
        // a position outside the table never reads out of bounds: its row comes out as NaN (as mi355_rope_apply)
        int64_t crow = pos[t];
        const bool bad_row = crow < 0 || crow >= table_rows;
        crow = bad_row ? 0 : crow;
        const float* cr = cosr + crow * D;
        const float* sr = sinr + crow * D;
        const u32x4 v1 = *reinterpret_cast<const u32x4*>(xr + j), v2 = *reinterpret_cast<const u32x4*>(xr + j + HALF);
        const f32x4 c1a = *reinterpret_cast<const f32x4*>(cr + j), c1b = *reinterpret_cast<const f32x4*>(cr + j + 4);
        const f32x4 c2a = *reinterpret_cast<const f32x4*>(cr + j + HALF), c2b = *reinterpret_cast<const f32x4*>(cr + j + HALF + 4);
        const f32x4 s1a = *reinterpret_cast<const f32x4*>(sr + j), s1b = *reinterpret_cast<const f32x4*>(sr + j + 4);
        const f32x4 s2a = *reinterpret_cast<const f32x4*>(sr + j + HALF), s2b = *reinterpret_cast<const f32x4*>(sr + j + HALF + 4);
        u32x4 o1, o2;
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
            float r1[2], r2[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int e = 2 * e2 + u;
                const float x1 = bf2f((bf16_t)(v1[e2] >> (16 * u))), x2 = bf2f((bf16_t)(v2[e2] >> (16 * u)));
                const float c1 = rnd_bf(e < 4 ? c1a[e & 3] : c1b[e & 3]), c2 = rnd_bf(e < 4 ? c2a[e & 3] : c2b[e & 3]);
                const float s1 = rnd_bf(e < 4 ? s1a[e & 3] : s1b[e & 3]), s2 = rnd_bf(e < 4 ? s2a[e & 3] : s2b[e & 3]);
                if (!BWD) {  // y = cos * x + sin * cat(-x2, x1)
                    r1[u] = rnd_bf(c1 * x1) + rnd_bf(s1 * (-x2));
                    r2[u] = rnd_bf(c2 * x2) + rnd_bf(s2 * x1);
                } else {  // dx = cos * dy + (z2, -z1), z = sin * dy
                    r1[u] = rnd_bf(c1 * x1) + rnd_bf(s2 * x2);
                    r2[u] = rnd_bf(c2 * x2) + (-rnd_bf(s1 * x1));
                }
                if (bad_row) r1[u] = r2[u] = __builtin_nanf("");
            }
            o1[e2] = pack_bf2(r1[0], r1[1]);
            o2[e2] = pack_bf2(r2[0], r2[1]);
        }
        *reinterpret_cast<u32x4*>(orow + j) = o1;
        *reinterpret_cast<u32x4*>(orow + j + HALF) = o2;
    }
}

// ------------------------------------------------------------------------------------------------ per-head maximum attention logit
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : fmaxf(a, b); }

// the maximum over the workgroup of a per-lane value, NaN winning; valid on thread 0
__device__ __forceinline__ float block_nan_max(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(red[0], red[1]), nan_max(red[2], red[3]));
}

// grid (ceil(S / 128), Hq, B); partial[h * parts + b * gridDim.x + blockIdx.x], parts = B * gridDim.x
template <int D>
__global__ __launch_bounds__(256) void max_logit_kernel(int S, int Hq, int Hkv, const bf16_t* __restrict__ q, int64_t ldq, const bf16_t* __restrict__ k,
                                                        int64_t ldk, const uint8_t* __restrict__ key_mask, float scale, float* __restrict__ partial) {
    using C = Tile32<D>;
    __shared__ __attribute__((aligned(16))) char kimg[C::IMG];
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.z, h = blockIdx.y, hkv = h / (Hq / Hkv);
    const int qb = blockIdx.x * 128;
    const int q0 = qb + wave * 32;
    const bool qvalid = q0 + (lane & 31) < S;
    const int query = qvalid ? q0 + (lane & 31) : -1;  // a row past S sees no key
    const int64_t tok0 = (int64_t)b * S;
    bf16x8 qf[C::KS];
    load_row_frags<D>(q + (tok0 + (qvalid ? query : 0)) * ldq + (int64_t)h * D, qvalid, lane, qf);
    float mx = NEG_INF;
    bool nan_seen = false;
    const int qlast = (qb + 127 < S ? qb + 127 : S - 1);
    for (int kt = 0; kt <= qlast / 32; ++kt) {  // tiles wholly above the workgroup's diagonal are not visited
        const int key0 = kt * 32;
        __syncthreads();
        load_tile<D, 256>(kimg, k + (tok0 + key0) * ldk + (int64_t)hkv * D, ldk, S - key0, threadIdx.x);
        __syncthreads();
        if (q0 >= S || key0 > q0 + 31) continue;  // above this wave's diagonal
        // bit kl of vis: key key0 + kl exists and is not masked
        const int mykey = key0 + (lane & 31);
        const bool kvis = mykey < S && (key_mask == nullptr || key_mask[tok0 + mykey] != 0);
        const unsigned vis = (unsigned)__ballot(kvis);
        if (vis == 0u) continue;
        f32x16 s;
        zero_tile(s);
        mma_rows<D>(s, kimg, qf, lane);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kl = acc_row(i, lane);
            const bool ok = ((vis >> kl) & 1u) && key0 + kl <= query;
            const float v = s[i] * scale;
            nan_seen |= ok && v != v;
            mx = fmaxf(mx, ok ? v : NEG_INF);
        }
    }
    if (nan_seen) mx = __builtin_nanf("");
    __syncthreads();
    mx = block_nan_max(mx, red);
    if (threadIdx.x == 0) partial[(int64_t)h * ((int64_t)gridDim.z * gridDim.x) + (int64_t)b * gridDim.x + blockIdx.x] = mx;
}

// out[h] = max of the head's `parts` partials (NaN wins); parts == 0 gives -inf.  grid Hq.
__global__ __launch_bounds__(256) void max_logit_fold_kernel(int64_t parts, const float* __restrict__ partial, float* __restrict__ out) {
    __shared__ float red[4];
    const float* row = partial + (int64_t)blockIdx.x * parts;
    float mx = NEG_INF;
    for (int64_t i = threadIdx.x; i < parts; i += 256) mx = nan_max(mx, row[i]);
    mx = block_nan_max(mx, red);
    if (threadIdx.x == 0) out[blockIdx.x] = mx;
}

// ------------------------------------------------------------------------------------------------ QK-Clip
// gamma of query head h (1 = no clip).  mode 0 per head, 1 naive (one gamma per layer), 2 magnitude.
__device__ __forceinline__ float clip_gamma(const float* __restrict__ m, int Hq, int h, float tau, int mode) {
    if (mode == 1) {
        float top = NEG_INF;
        bool nan_seen = false;
        for (int i = 0; i < Hq; ++i) {
            nan_seen |= m[i] != m[i];
            top = fmaxf(top, m[i]);
        }
        return (!nan_seen && top > tau && top > 0.f && top < __builtin_huge_valf()) ? tau / top : 1.f;
    }
    const float v = mode == 2 ? fabsf(m[h]) : m[h];
    return (v > tau && v > 0.f && v < __builtin_huge_valf()) ? tau / v : 1.f;  // false for NaN
}

__device__ __forceinline__ float clip_pow(float g, float e) { return e == 0.5f ? sqrtf(g) : powf(g, e); }

// grid (chunks, Hq + Hkv): head blockIdx.y of [W_q ; W_k], `per_head` = D * d_in elements each
template <bool VEC>
__global__ __launch_bounds__(256) void qk_clip_kernel(int Hq, int Hkv, int64_t per_head, bf16_t* __restrict__ wq, bf16_t* __restrict__ wk,
                                                      const float* __restrict__ m, float tau, float alpha, int mode) {
    const int hh = blockIdx.y;
    float s;
    bf16_t* w;
    if (hh < Hq) {
        const float g = clip_gamma(m, Hq, hh, tau, mode);
        if (g >= 1.f) return;
        s = clip_pow(g, alpha);
        w = wq + (int64_t)hh * per_head;
    } else {
        const int g0 = hh - Hq, rep = Hq / Hkv;
        float g = 1.f;
        for (int r = 0; r < rep; ++r) g = fminf(g, clip_gamma(m, Hq, g0 * rep + r, tau, mode));  // the strongest clip of the group
        if (g >= 1.f) return;
        s = clip_pow(g, 1.f - alpha);
        w = wk + (int64_t)g0 * per_head;
    }
    if (VEC) {
        const int64_t n8 = per_head / 8;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
            u32x4 v = *reinterpret_cast<const u32x4*>(w + 8 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = pack_bf2(bf2f((bf16_t)(v[e] & 0xffffu)) * s, bf2f((bf16_t)(v[e] >> 16)) * s);
            *reinterpret_cast<u32x4*>(w + 8 * i) = v;
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per_head; i += (int64_t)gridDim.x * 256) w[i] = f2bf(bf2f(w[i]) * s);
    }
}

int check_heads(const char* who, int Hq, int Hkv, int D) {
    MI355_REQUIRE(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "%s: query heads (%d) must be a multiple of kv heads (%d)", who, Hq, Hkv);
    MI355_REQUIRE(Hq <= 65535, "%s: at most 65535 query heads", who);
    MI355_REQUIRE(D == 64 || D == 128, "%s: head_dim %d not built (64, 128)", who, D);
    return 0;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" int mi355_llama_rope_fwd(int64_t tokens, int Hq, int Hkv, int D, const void* qkv, int64_t ldqkv, const float* cos_t, const float* sin_t,
                                    int64_t table_rows, const int32_t* pos, void* q, void* k, void* stream) {
    if (check_heads("mi355_llama_rope_fwd", Hq, Hkv, D)) return 1;
    MI355_REQUIRE(tokens >= 0 && tokens <= ((int64_t)1 << 40), "mi355_llama_rope_fwd: bad token count");
    if (tokens == 0) return 0;
    MI355_REQUIRE(qkv && cos_t && sin_t && pos && q && k, "mi355_llama_rope_fwd: null pointer");
    MI355_REQUIRE(table_rows > 0, "mi355_llama_rope_fwd: empty coefficient table");
    MI355_REQUIRE(ldqkv >= (int64_t)(Hq + 2 * Hkv) * D && ldqkv % 8 == 0, "mi355_llama_rope_fwd: ldqkv must be a multiple of 8, at least (Hq + 2 Hkv) * D");
    MI355_REQUIRE(aligned16({qkv, cos_t, sin_t, q, k}), "mi355_llama_rope_fwd: qkv, cos, sin, q, k must be 16-byte aligned");
    const bf16_t* x = (const bf16_t*)qkv;
    const int grid = flat_grid(tokens * (Hq + Hkv) * (D / 16));
#define LAUNCH(DD) llama_rope_kernel<DD, false><<<grid, 256, 0, ST(stream)>>>(tokens, Hq, Hkv, x, ldqkv, x + (int64_t)Hq * D, ldqkv, cos_t, sin_t, table_rows, pos, \
                                                                              (bf16_t*)q, (int64_t)Hq * D, (bf16_t*)k, (int64_t)Hkv * D)
    if (D == 64) LAUNCH(64); else LAUNCH(128);
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_llama_rope_fwd");
    return 0;
}

extern "C" int mi355_llama_rope_bwd(int64_t tokens, int Hq, int Hkv, int D, const void* dq, int64_t lddq, const void* dk, int64_t lddk, const float* cos_t,
                                    const float* sin_t, int64_t table_rows, const int32_t* pos, void* dqkv, int64_t lddqkv, void* stream) {
    if (check_heads("mi355_llama_rope_bwd", Hq, Hkv, D)) return 1;
    MI355_REQUIRE(tokens >= 0 && tokens <= ((int64_t)1 << 40), "mi355_llama_rope_bwd: bad token count");
    if (tokens == 0) return 0;
    MI355_REQUIRE(dq && dk && cos_t && sin_t && pos && dqkv, "mi355_llama_rope_bwd: null pointer");
    MI355_REQUIRE(table_rows > 0, "mi355_llama_rope_bwd: empty coefficient table");
    MI355_REQUIRE(lddq >= (int64_t)Hq * D && lddk >= (int64_t)Hkv * D && lddqkv >= (int64_t)(Hq + Hkv) * D,
                  "mi355_llama_rope_bwd: leading dimension smaller than heads*head_dim");
    MI355_REQUIRE(lddq % 8 == 0 && lddk % 8 == 0 && lddqkv % 8 == 0, "mi355_llama_rope_bwd: leading dimensions must be multiples of 8 elements");
    MI355_REQUIRE(aligned16({dq, dk, cos_t, sin_t, dqkv}), "mi355_llama_rope_bwd: dq, dk, cos, sin, dqkv must be 16-byte aligned");
    bf16_t* o = (bf16_t*)dqkv;
    const int grid = flat_grid(tokens * (Hq + Hkv) * (D / 16));
#define LAUNCH(DD) llama_rope_kernel<DD, true><<<grid, 256, 0, ST(stream)>>>(tokens, Hq, Hkv, (const bf16_t*)dq, lddq, (const bf16_t*)dk, lddk, cos_t, sin_t, table_rows, \
                                                                             pos, o, lddqkv, o + (int64_t)Hq * D, lddqkv)
    if (D == 64) LAUNCH(64); else LAUNCH(128);
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_llama_rope_bwd");
    return 0;
}

extern "C" int64_t mi355_attn_max_logit_partials(int B, int S, int Hq) {
    if (B <= 0 || S <= 0 || Hq <= 0) return 0;
    return (int64_t)Hq * B * (((int64_t)S + 127) / 128);
}

extern "C" int mi355_attn_max_logit(int B, int S, int Hq, int Hkv, int D, const void* q, int64_t ldq, const void* k, int64_t ldk, const uint8_t* key_mask,
                                    float scale, float* partial, int64_t partial_elems, float* out, void* stream) {
    if (check_heads("mi355_attn_max_logit", Hq, Hkv, D)) return 1;
    MI355_REQUIRE(B >= 0 && S >= 0, "mi355_attn_max_logit: negative batch or sequence length");
    MI355_REQUIRE(B <= 65535 && S <= (1 << 30) - 64, "mi355_attn_max_logit: grid limits (B <= 65535, S <= 2^30 - 64)");
    MI355_REQUIRE(out, "mi355_attn_max_logit: null pointer");
    const int64_t parts = (B == 0 || S == 0) ? 0 : (int64_t)B * ((S + 127) / 128);
    if (parts) {
        MI355_REQUIRE(q && k && partial, "mi355_attn_max_logit: null pointer");
        MI355_REQUIRE(partial_elems >= parts * Hq, "mi355_attn_max_logit: partial holds %lld floats, %lld needed (mi355_attn_max_logit_partials)",
                      (long long)partial_elems, (long long)(parts * Hq));
        MI355_REQUIRE(ldq >= (int64_t)Hq * D && ldk >= (int64_t)Hkv * D, "mi355_attn_max_logit: leading dimension smaller than heads*head_dim");
        MI355_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0, "mi355_attn_max_logit: leading dimensions must be multiples of 8 elements");
        MI355_REQUIRE(aligned16({q, k}), "mi355_attn_max_logit: q, k must be 16-byte aligned");
        dim3 grid((S + 127) / 128, Hq, B);
        if (D == 64) max_logit_kernel<64><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale, partial);
        else max_logit_kernel<128><<<grid, 256, 0, ST(stream)>>>(S, Hq, Hkv, (const bf16_t*)q, ldq, (const bf16_t*)k, ldk, key_mask, scale, partial);
        MI355_LAUNCH_CHECK("mi355_attn_max_logit");
    }
    max_logit_fold_kernel<<<Hq, 256, 0, ST(stream)>>>(parts, partial, out);
    MI355_LAUNCH_CHECK("mi355_attn_max_logit (fold)");
    return 0;
}

extern "C" int mi355_qk_clip(int Hq, int Hkv, int D, int64_t d_in, void* wq, void* wk, const float* max_logits, float tau, float alpha, int mode,
                             void* stream) {
    MI355_REQUIRE(Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "mi355_qk_clip: query heads (%d) must be a multiple of kv heads (%d)", Hq, Hkv);
    MI355_REQUIRE(Hq + (int64_t)Hkv <= 65535, "mi355_qk_clip: at most 65535 heads");
    MI355_REQUIRE(D > 0 && d_in > 0 && d_in <= ((int64_t)1 << 40) / D, "mi355_qk_clip: bad head_dim %d or d_in %lld", D, (long long)d_in);
    MI355_REQUIRE(mode >= 0 && mode <= 2, "mi355_qk_clip: mode %d (0 per head, 1 naive, 2 magnitude)", mode);
    MI355_REQUIRE(mode != 2 || Hq == Hkv, "mi355_qk_clip: the magnitude mode is defined for multi-head attention only (Hq == Hkv)");
    MI355_REQUIRE(tau > 0.f && alpha >= 0.f && alpha <= 1.f, "mi355_qk_clip: threshold must be positive and alpha in [0, 1]");
    MI355_REQUIRE(wq && wk && max_logits, "mi355_qk_clip: null pointer");
    MI355_REQUIRE(((uintptr_t)wq & 1) == 0 && ((uintptr_t)wk & 1) == 0, "mi355_qk_clip: weights must be 2-byte aligned");
    const int64_t per_head = (int64_t)D * d_in;
    const bool vec = per_head % 8 == 0 && aligned16({wq, wk});
    int64_t chunks = (per_head / (vec ? 8 : 1) + 1023) / 1024;  // four elements (or vectors) per thread
    chunks = chunks < 1 ? 1 : (chunks > 1024 ? 1024 : chunks);
    dim3 grid((unsigned)chunks, Hq + Hkv);
    if (vec) qk_clip_kernel<true><<<grid, 256, 0, ST(stream)>>>(Hq, Hkv, per_head, (bf16_t*)wq, (bf16_t*)wk, max_logits, tau, alpha, mode);
    else qk_clip_kernel<false><<<grid, 256, 0, ST(stream)>>>(Hq, Hkv, per_head, (bf16_t*)wq, (bf16_t*)wk, max_logits, tau, alpha, mode);
    MI355_LAUNCH_CHECK("mi355_qk_clip");
    return 0;
}
