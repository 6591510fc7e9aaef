// Gemma3 (reference llama3_to_gemma3/): the three row kernels the family needs beside what exists.  Its sliding-window attention
// (mi355_swa_attn_fwd / _bwd) is the banded family of attention_band.hip, called with DV = D and no sink.
//
// Row kernels (one wave per row, fp32 math, one rounding at the output; parameter gradients as per-workgroup partial rows for
// mi355_reduce_rows_f32):
//   Gemma RMSNorm (gemma3_transformer_block.py:14-37): y = scale * x / (sqrt(mean(x^2)) + eps) -- eps is added to the RMS, not under the root.
//   RoPE + per-head LayerNorm (gemma3_attention.py:203-207, 13-43): half-split rotation with bf16-rounded cos / sin, then
//     (r - mean) / (std + eps) * scale + shift over head_dim, population std; one scale / shift pair for the query heads, one for the key heads.
//   GeGLU (gemma3_transformer_block.py:101-106): a = lin1 * gelu_erf(lin_gate) on the fused [T, 2F] projection.
#include "host_checks.h"
#include "rows_bf16.h"

namespace {

// ------------------------------------------------------------------------------------------------ Gemma RMSNorm
__global__ __launch_bounds__(256) void g3_rmsnorm_fwd_kernel(int64_t rows, int width, const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                             const bf16_t* __restrict__ w, bf16_t* __restrict__ y, float eps) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nvec = width >> 3;
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < rows; row += (int64_t)gridDim.x * 4) {
        float ss = 0.f;
        for (int i = lane; i < nvec; i += 64) {
            float xv[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + row * width + i * 8), xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += xv[e] * xv[e];
        }
        const float a = 1.0f / (sqrtf(wave_sum(ss) / (float)width) + eps);
        for (int i = lane; i < nvec; i += 64) {
            float xv[8], wf[8], o[8], rs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            unpack8(*reinterpret_cast<const u32x4*>(x + row * width + i * 8), xv);
            unpack8(*reinterpret_cast<const u32x4*>(w + i * 8), wf);
            if (res) unpack8(*reinterpret_cast<const u32x4*>(res + row * width + i * 8), rs);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = wf[e] * (xv[e] * a) + rs[e];
            *reinterpret_cast<u32x4*>(y + row * width + i * 8) = pack8(o);
        }
    }
}

// y = w x a, a = 1 / (r + eps), r = sqrt(mean x^2):  dx = a g - a^2 x <g, x> / (width r), g = w dy  (the second term is 0 for an all-zero row:
// |x| / r is bounded and <g, x> = 0);  dw = sum over rows of dy x a.
__global__ __launch_bounds__(256) void g3_rmsnorm_bwd_kernel(int64_t rows, int width, const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                             const bf16_t* __restrict__ dy, const bf16_t* __restrict__ dres, bf16_t* __restrict__ dx,
                                                             float* __restrict__ dw_partial, float eps) {
    extern __shared__ __attribute__((aligned(16))) float g3_dw_lds[];  // [4][width]: one region per wave, summed in a fixed order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nvec = width >> 3;
    float* dw_mine = g3_dw_lds + wv * width;  // element i*8+e is touched by lane i % 64 of this wave only: plain adds
    for (int i = threadIdx.x; i < 4 * width; i += 256) g3_dw_lds[i] = 0.f;
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < rows; row += (int64_t)gridDim.x * 4) {
        float ss = 0.f, dot = 0.f;
        for (int i = lane; i < nvec; i += 64) {
            float xv[8], dyv[8], wf[8];
            unpack8(*reinterpret_cast<const u32x4*>(x + row * width + i * 8), xv);
            unpack8(*reinterpret_cast<const u32x4*>(dy + row * width + i * 8), dyv);
            unpack8(*reinterpret_cast<const u32x4*>(w + i * 8), wf);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ss += xv[e] * xv[e];
                dot += dyv[e] * wf[e] * xv[e];
            }
        }
        const float r = sqrtf(wave_sum(ss) / (float)width);
        const float a = 1.0f / (r + eps);
        dot = wave_sum(dot);
        const float coef = r > 0.f ? a * a * dot / ((float)width * r) : 0.f;
        for (int i = lane; i < nvec; i += 64) {
            float xv[8], dyv[8], wf[8], o[8], rs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            unpack8(*reinterpret_cast<const u32x4*>(x + row * width + i * 8), xv);
            unpack8(*reinterpret_cast<const u32x4*>(dy + row * width + i * 8), dyv);
            unpack8(*reinterpret_cast<const u32x4*>(w + i * 8), wf);
            if (dres) unpack8(*reinterpret_cast<const u32x4*>(dres + row * width + i * 8), rs);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = a * dyv[e] * wf[e] - coef * xv[e] + rs[e];
                dw_mine[i * 8 + e] += dyv[e] * xv[e] * a;
            }
            *reinterpret_cast<u32x4*>(dx + row * width + i * 8) = pack8(o);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < width; i += 256)
        dw_partial[(int64_t)blockIdx.x * width + i] = ((g3_dw_lds[i] + g3_dw_lds[width + i]) + g3_dw_lds[2 * width + i]) + g3_dw_lds[3 * width + i];
}

// ------------------------------------------------------------------------------------------------ RoPE + per-head LayerNorm
// A row is one (token, head), head < Hq a query head, else a key head; a lane owns feature j of the first half and its partner j + D/2, so a wave
// covers 128 / D rows at a time and the row sums are shuffles among the D/2 lanes of a row.
template <int HALF>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = HALF / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int D, bool BWD>
__global__ __launch_bounds__(256) void g3_rope_ln_kernel(int64_t tokens, int S, int Hq, int Hkv, const bf16_t* __restrict__ x, int64_t ldx,
                                                         const float* __restrict__ cos_t, const float* __restrict__ sin_t,
                                                         const bf16_t* __restrict__ q_scale, const bf16_t* __restrict__ q_shift,
                                                         const bf16_t* __restrict__ k_scale, const bf16_t* __restrict__ k_shift,
                                                         const bf16_t* __restrict__ dy, int64_t lddy, bf16_t* __restrict__ out, int64_t ldo,
                                                         float* __restrict__ partial, float eps) {
    constexpr int HALF = D / 2, RPW = 64 / HALF;
    __shared__ float acc_lds[4][RPW][4][D];  // [wave][row of the wave][q scale, q shift, k scale, k shift][feature]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int sub = lane / HALF, j = lane % HALF;
    const int H = Hq + Hkv;
    const int64_t total = tokens * H;
    const int64_t groups = (total + RPW - 1) / RPW;
    const float qs1 = bf2f(q_scale[j]), qs2 = bf2f(q_scale[j + HALF]), ks1 = bf2f(k_scale[j]), ks2 = bf2f(k_scale[j + HALF]);
    const float qb1 = bf2f(q_shift[j]), qb2 = bf2f(q_shift[j + HALF]), kb1 = bf2f(k_shift[j]), kb2 = bf2f(k_shift[j + HALF]);
    float g_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // q scale (j, j+HALF), q shift, k scale, k shift
    for (int64_t g = (int64_t)blockIdx.x * 4 + wv; g < groups; g += (int64_t)gridDim.x * 4) {
        const int64_t row = g * RPW + sub;
        const bool valid = row < total;
        const int64_t t = valid ? row / H : 0;
        const int h = valid ? (int)(row % H) : 0;
        const bool is_q = h < Hq;
        const int pos = (int)(t % S);
        float x1 = 0.f, x2 = 0.f;
        if (valid) {
            x1 = bf2f(x[t * ldx + (int64_t)h * D + j]);
            x2 = bf2f(x[t * ldx + (int64_t)h * D + j + HALF]);
        }
        const float c1 = rbf(cos_t[(int64_t)pos * D + j]), c2 = rbf(cos_t[(int64_t)pos * D + j + HALF]);
        const float s1 = rbf(sin_t[(int64_t)pos * D + j]), s2 = rbf(sin_t[(int64_t)pos * D + j + HALF]);
        const float r1 = c1 * x1 - s1 * x2, r2 = c2 * x2 + s2 * x1;  // cos * x + sin * cat(-x2, x1)
        const float mu = group_sum<HALF>(r1 + r2) / (float)D;
        const float e1 = r1 - mu, e2 = r2 - mu;
        const float sd = sqrtf(group_sum<HALF>(e1 * e1 + e2 * e2) / (float)D);
        const float a = 1.0f / (sd + eps);
        const float sc1 = is_q ? qs1 : ks1, sc2 = is_q ? qs2 : ks2;
        if (!BWD) {
            if (valid) {
                out[t * ldo + (int64_t)h * D + j] = f2bf(e1 * a * sc1 + (is_q ? qb1 : kb1));
                out[t * ldo + (int64_t)h * D + j + HALF] = f2bf(e2 * a * sc2 + (is_q ? qb2 : kb2));
            }
        } else {
            float d1 = 0.f, d2 = 0.f;
            if (valid) {
                d1 = bf2f(dy[t * lddy + (int64_t)h * D + j]);
                d2 = bf2f(dy[t * lddy + (int64_t)h * D + j + HALF]);
            }
            const float g1 = d1 * sc1, g2 = d2 * sc2;
            const float mg = group_sum<HALF>(g1 + g2) / (float)D;
            const float gd = group_sum<HALF>(g1 * e1 + g2 * e2);
            const float coef = sd > 0.f ? a * a * gd / ((float)D * sd) : 0.f;
            const float dr1 = a * (g1 - mg) - coef * e1, dr2 = a * (g2 - mg) - coef * e2;
            if (valid) {  // the adjoint of the rotation: dx = cos * dr + (z2, -z1), z = sin * dr
                out[t * ldo + (int64_t)h * D + j] = f2bf(c1 * dr1 + s2 * dr2);
                out[t * ldo + (int64_t)h * D + j + HALF] = f2bf(c2 * dr2 - s1 * dr1);
                const int o = is_q ? 0 : 4;
                g_acc[o] += d1 * e1 * a;
                g_acc[o + 1] += d2 * e2 * a;
                g_acc[o + 2] += d1;
                g_acc[o + 3] += d2;
            }
        }
    }
    if (BWD) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            acc_lds[wv][sub][c][j] = g_acc[2 * c];
            acc_lds[wv][sub][c][j + HALF] = g_acc[2 * c + 1];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * D; i += 256) {
            float s = 0.f;
            for (int w = 0; w < 4; ++w)
                for (int r = 0; r < RPW; ++r) s += acc_lds[w][r][i / D][i % D];
            partial[(int64_t)blockIdx.x * 4 * D + i] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ GeGLU
// gelu(g) = g Phi(g) with Phi(g) = erfc(-g / sqrt 2) / 2: no cancellation in the left tail
__device__ __forceinline__ float norm_cdf(float g) { return 0.5f * erfcf(-g * 0.70710678118654752440f); }

__global__ __launch_bounds__(256) void g3_geglu_fwd_kernel(int64_t tokens, int F, const bf16_t* __restrict__ gu, bf16_t* __restrict__ a) {
    const int fv = F >> 3;
    const int64_t total = tokens * fv;
    for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < total; item += (int64_t)gridDim.x * 256) {
        const int64_t t = item / fv;
        const int c = (int)(item % fv) * 8;
        float u[8], g[8], o[8];
        unpack8(*reinterpret_cast<const u32x4*>(gu + t * 2 * F + c), u);
        unpack8(*reinterpret_cast<const u32x4*>(gu + t * 2 * F + F + c), g);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = u[e] * g[e] * norm_cdf(g[e]);
        *reinterpret_cast<u32x4*>(a + t * F + c) = pack8(o);
    }
}

__global__ __launch_bounds__(256) void g3_geglu_bwd_kernel(int64_t tokens, int F, const bf16_t* __restrict__ gu, const bf16_t* __restrict__ da,
                                                           bf16_t* __restrict__ dgu) {
    const int fv = F >> 3;
    const int64_t total = tokens * fv;
    for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < total; item += (int64_t)gridDim.x * 256) {
        const int64_t t = item / fv;
        const int c = (int)(item % fv) * 8;
        float u[8], g[8], d[8], du[8], dg[8];
        unpack8(*reinterpret_cast<const u32x4*>(gu + t * 2 * F + c), u);
        unpack8(*reinterpret_cast<const u32x4*>(gu + t * 2 * F + F + c), g);
        unpack8(*reinterpret_cast<const u32x4*>(da + t * F + c), d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float cdf = norm_cdf(g[e]);
            du[e] = d[e] * g[e] * cdf;
            dg[e] = d[e] * u[e] * (cdf + g[e] * 0.3989422804014327f * __expf(-0.5f * g[e] * g[e]));
        }
        *reinterpret_cast<u32x4*>(dgu + t * 2 * F + c) = pack8(du);
        *reinterpret_cast<u32x4*>(dgu + t * 2 * F + F + c) = pack8(dg);
    }
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

extern "C" int mi355_g3_rmsnorm_fwd(int64_t rows, int width, const void* x, const void* residual, const void* scale, void* y, float eps, void* stream) {
    MI355_REQUIRE(rows >= 0 && width > 0 && (width & 7) == 0, "mi355_g3_rmsnorm_fwd: width must be a positive multiple of 8 (got %d)", width);
    if (rows == 0) return 0;
    MI355_REQUIRE(x && scale && y, "mi355_g3_rmsnorm_fwd: null pointer");
    MI355_REQUIRE(aligned16({x, residual, scale, y}), "mi355_g3_rmsnorm_fwd: operands must be 16-byte aligned");
    g3_rmsnorm_fwd_kernel<<<row_grid(rows), 256, 0, ST(stream)>>>(rows, width, (const bf16_t*)x, (const bf16_t*)residual, (const bf16_t*)scale, (bf16_t*)y, eps);
    MI355_LAUNCH_CHECK("mi355_g3_rmsnorm_fwd");
    return 0;
}

extern "C" int mi355_g3_rmsnorm_bwd(int64_t rows, int width, const void* x, const void* scale, const void* dy, const void* dres, void* dx,
                                    float* dscale_partial, int parts, float eps, void* stream) {
    MI355_REQUIRE(rows > 0 && width > 0 && (width & 7) == 0 && width <= 4096,
                  "mi355_g3_rmsnorm_bwd: bad rows / width %d (multiple of 8, <= 4096: four per-wave LDS regions of width floats)", width);
    MI355_REQUIRE(parts > 0 && parts <= 65535, "mi355_g3_rmsnorm_bwd: parts must be in 1..65535 (got %d)", parts);
    MI355_REQUIRE(x && scale && dy && dx && dscale_partial, "mi355_g3_rmsnorm_bwd: null pointer");
    MI355_REQUIRE(aligned16({x, scale, dy, dres, dx}), "mi355_g3_rmsnorm_bwd: operands must be 16-byte aligned");
    g3_rmsnorm_bwd_kernel<<<parts, 256, 4 * width * sizeof(float), ST(stream)>>>(rows, width, (const bf16_t*)x, (const bf16_t*)scale, (const bf16_t*)dy,
                                                                                 (const bf16_t*)dres, (bf16_t*)dx, dscale_partial, eps);
    MI355_LAUNCH_CHECK("mi355_g3_rmsnorm_bwd");
    return 0;
}

static int check_rope_ln(const char* who, int64_t tokens, int S, int Hq, int Hkv, int D, int64_t ldx, int64_t ldy, int64_t table_rows) {
    MI355_REQUIRE(tokens >= 0 && S > 0 && Hq >= 0 && Hkv >= 0 && Hq + Hkv > 0, "%s: bad token / head counts", who);
    MI355_REQUIRE(D == 32 || D == 64 || D == 128, "%s: head_dim %d not built (32, 64, 128)", who, D);
    MI355_REQUIRE(ldx >= (int64_t)(Hq + Hkv) * D && ldy >= (int64_t)(Hq + Hkv) * D, "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(table_rows >= S, "%s: coefficient table has %lld rows, sequence length is %d", who, (long long)table_rows, S);
    return 0;
}

extern "C" int mi355_g3_rope_ln_fwd(int64_t tokens, int S, int Hq, int Hkv, int D, const void* x, int64_t ldx, const float* cos_t, const float* sin_t,
                                    int64_t table_rows, const void* q_scale, const void* q_shift, const void* k_scale, const void* k_shift, void* y,
                                    int64_t ldy, float eps, void* stream) {
    if (check_rope_ln("mi355_g3_rope_ln_fwd", tokens, S, Hq, Hkv, D, ldx, ldy, table_rows)) return 1;
    if (tokens == 0) return 0;
    MI355_REQUIRE(x && cos_t && sin_t && q_scale && q_shift && k_scale && k_shift && y, "mi355_g3_rope_ln_fwd: null pointer");
    const int grid = row_grid(tokens * (Hq + Hkv) / (128 / D) + 1);
#define LAUNCH(DD)                                                                                                                                      \
    g3_rope_ln_kernel<DD, false><<<grid, 256, 0, ST(stream)>>>(tokens, S, Hq, Hkv, (const bf16_t*)x, ldx, cos_t, sin_t, (const bf16_t*)q_scale,           \
                                                              (const bf16_t*)q_shift, (const bf16_t*)k_scale, (const bf16_t*)k_shift, nullptr, 0, (bf16_t*)y, \
                                                              ldy, nullptr, eps)
    switch (D) {
        case 32: LAUNCH(32); break;
        case 64: LAUNCH(64); break;
        default: LAUNCH(128); break;
    }
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_g3_rope_ln_fwd");
    return 0;
}

extern "C" int mi355_g3_rope_ln_bwd(int64_t tokens, int S, int Hq, int Hkv, int D, const void* x, int64_t ldx, const float* cos_t, const float* sin_t,
                                    int64_t table_rows, const void* q_scale, const void* q_shift, const void* k_scale, const void* k_shift, const void* dy,
                                    int64_t lddy, void* dx, int64_t lddx, float* partial, int parts, float eps, void* stream) {
    if (check_rope_ln("mi355_g3_rope_ln_bwd", tokens, S, Hq, Hkv, D, ldx, lddy, table_rows)) return 1;
    MI355_REQUIRE(lddx >= (int64_t)(Hq + Hkv) * D, "mi355_g3_rope_ln_bwd: leading dimension smaller than heads*head_dim");
    MI355_REQUIRE(tokens > 0 && parts > 0 && parts <= 65535, "mi355_g3_rope_ln_bwd: tokens must be positive and parts in 1..65535 (got %d)", parts);
    MI355_REQUIRE(x && cos_t && sin_t && q_scale && q_shift && k_scale && k_shift && dy && dx && partial, "mi355_g3_rope_ln_bwd: null pointer");
#define LAUNCH(DD)                                                                                                                                      \
    g3_rope_ln_kernel<DD, true><<<parts, 256, 0, ST(stream)>>>(tokens, S, Hq, Hkv, (const bf16_t*)x, ldx, cos_t, sin_t, (const bf16_t*)q_scale,           \
                                                              (const bf16_t*)q_shift, (const bf16_t*)k_scale, (const bf16_t*)k_shift, (const bf16_t*)dy,  \
                                                              lddy, (bf16_t*)dx, lddx, partial, eps)
    switch (D) {
        case 32: LAUNCH(32); break;
        case 64: LAUNCH(64); break;
        default: LAUNCH(128); break;
    }
#undef LAUNCH
    MI355_LAUNCH_CHECK("mi355_g3_rope_ln_bwd");
    return 0;
}

extern "C" int mi355_geglu_fwd(int64_t tokens, int F, const void* gu, void* a, void* stream) {
    MI355_REQUIRE(tokens >= 0 && F > 0 && (F & 7) == 0, "mi355_geglu_fwd: F must be a positive multiple of 8 (got %d)", F);
    if (tokens == 0) return 0;
    MI355_REQUIRE(gu && a, "mi355_geglu_fwd: null pointer");
    MI355_REQUIRE(aligned16({gu, a}), "mi355_geglu_fwd: operands must be 16-byte aligned");
    g3_geglu_fwd_kernel<<<flat_grid(tokens * (F >> 3)), 256, 0, ST(stream)>>>(tokens, F, (const bf16_t*)gu, (bf16_t*)a);
    MI355_LAUNCH_CHECK("mi355_geglu_fwd");
    return 0;
}

extern "C" int mi355_geglu_bwd(int64_t tokens, int F, const void* gu, const void* da, void* dgu, void* stream) {
    MI355_REQUIRE(tokens >= 0 && F > 0 && (F & 7) == 0, "mi355_geglu_bwd: F must be a positive multiple of 8 (got %d)", F);
    if (tokens == 0) return 0;
    MI355_REQUIRE(gu && da && dgu, "mi355_geglu_bwd: null pointer");
    MI355_REQUIRE(aligned16({gu, da, dgu}), "mi355_geglu_bwd: operands must be 16-byte aligned");
    g3_geglu_bwd_kernel<<<flat_grid(tokens * (F >> 3)), 256, 0, ST(stream)>>>(tokens, F, (const bf16_t*)gu, (const bf16_t*)da, (bf16_t*)dgu);
    MI355_LAUNCH_CHECK("mi355_geglu_bwd");
    return 0;
}
