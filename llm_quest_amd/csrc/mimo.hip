// MiMo-V2-Flash (reference xiaomi/): the per-head RMSNorm + partial RoPE of the q and k heads.  Its attention with a learnable sink and decoupled
// q/k and v head dims (mi355_sink_attn_fwd / _bwd), and the sink's gradient, are the banded family of attention_band.hip.
//
// Norm + partial RoPE (mimo_v2_flash_attention.py:88-94): n = x rsqrt(mean(x^2) + eps) w over head_dim (torch.nn.RMSNorm in fp32), then the half-split
// rotation of the first R features, pairs (d, d + R/2), cos / sin rounded to bf16; features >= R pass through.  One wave per (token, head) row,
// fp32 math, one rounding at the output; R is any even number in [2, D].
#include "host_checks.h"
#include "rows_bf16.h"

namespace {

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
int check_normrope(const char* who, int64_t tokens, int S, int Hq, int Hkv, int D, int R, int64_t ldx, int64_t ldy, int64_t table_rows) {
    MI355_REQUIRE(tokens >= 0 && tokens <= ((int64_t)1 << 40) && S > 0 && Hq >= 0 && Hkv >= 0 && Hq <= 65535 && Hkv <= 65535 && Hq + Hkv > 0,
                  "%s: bad token / head counts", who);
    MI355_REQUIRE(D == 64 || D == 128 || D == 192, "%s: head_dim %d not built (64, 128, 192)", who, D);
    MI355_REQUIRE(R >= 2 && R <= D && R % 2 == 0, "%s: rotated width %d must be even and in [2, head_dim = %d]", who, R, D);
    MI355_REQUIRE(ldx >= (int64_t)(Hq + Hkv) * D && ldy >= (int64_t)(Hq + Hkv) * D, "%s: leading dimension smaller than heads*head_dim", who);
    MI355_REQUIRE(table_rows >= S, "%s: coefficient table has %lld rows, sequence length is %d", who, (long long)table_rows, S);
    return 0;
}

}  // namespace

#define ST(s) ((hipStream_t)(s))

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
