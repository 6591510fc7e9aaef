// Nemotron-3 LatentMoE (reference llm_quest/moe/nvidia_latent_moe.py:89-135): what the layer needs beyond the kernels of moe.hip and deepseek_moe.hip.
//
//   route     sigmoid (not softmax) of the E gate logits of a token, selection of the k largest (probability + balancing bias) keys (ties: the lower
//             expert index), weights from the UNBIASED probabilities, renormalised and times the routed scaling factor; or, with a forced
//             selection, the weights of the given experts.  And its backward: a sigmoid does not couple experts, so only the selected ones get a gradient.
//   relu2     the squared-ReLU gated activation between an expert's two products (routed experts at the latent width, the shared expert at full width),
//             forward and backward, over [R, 2F] rows [u | g] = [lin1 | lin_gate]
//
// The plan, the row dispatch, the combine and its backward are moe.hip's, the bias update deepseek_moe.hip's; limits, host checks and the bias-balanced selection
// loop (shared with deepseek_moe.hip's router) are moe_common.h's.
// No atomics, one writer per element, fixed summation orders.  Rounding points are the reference's bf16 tensors:
//   p = bf16(sigmoid), key = p + biases in the promoted dtype, s = bf16(sum_j v_j), w_j = bf16(bf16(v_j / s) * scaling)   (nvidia_latent_moe.py:101-108)
//   q = bf16(bf16(relu(g))^2), a = bf16(u * q)                                                                            (nvidia_latent_moe.py:14, 39-44)
// The activation is a kernel of its own and no epilogue of the gate-up product: gemm.hip is part of the headline step's source fingerprint.
#include "moe_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ route, forward
// One wave per token; lane l holds experts l and l + 64.  Columns at and beyond E are never read.
template <bool BIAS_F32, bool FORCED>
__global__ __launch_bounds__(256) void latmoe_route_fwd_kernel(int64_t T, int E, int k, const bf16_t* __restrict__ logits, int64_t ldl, const void* __restrict__ bias,
                                                               const int* __restrict__ forced, float scaling, bf16_t* __restrict__ p, int64_t ldp, int* __restrict__ idx,
                                                               bf16_t* __restrict__ w, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    float bv[2] = {0.f, 0.f};
    if (!FORCED) route_load_bias<BIAS_F32>(bias, E, lane, bv);
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        float pf[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pf[h] = 0.f;
            if (lane + 64 * h < E) {
                const bf16_t pb = f2bf(1.0f / (1.0f + expf(-bf2f(logits[t * ldl + lane + 64 * h]))));
                pf[h] = bf2f(pb);
                p[t * ldp + lane + 64 * h] = pb;
            }
        }
        float v[MOE_MAX_K];
        int ex[MOE_MAX_K];
        const float sum = route_select_biased<BIAS_F32, FORCED>(pf, bv, FORCED ? forced + t * k : nullptr, E, k, lane, ex, v);  // the selection is DeepSeekMoE's
        const float sr = rbf(sum);
        if (lane == 0) {
            s[t] = sr;
#pragma unroll
            for (int j = 0; j < MOE_MAX_K; ++j)
                if (j < k) {
                    idx[t * k + j] = ex[j];
                    w[t * k + j] = f2bf(rbf(v[j] / sr) * scaling);  // the division and the in-place scaling each round (nvidia_latent_moe.py:107-108)
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------ route, backward
// w_j = scaling v_j / s, s = sum_i v_i:  dv_j = scaling (dw_j - sum_i dw_i v_i / s) / s;  dlogits_e = bf16(dv_j p_e (1 - p_e)) for e = idx_j, else exactly 0.
__global__ __launch_bounds__(256) void latmoe_route_bwd_kernel(int64_t T, int E, int k, const float* __restrict__ dw, const float* __restrict__ s,
                                                               const int* __restrict__ idx, const bf16_t* __restrict__ p, int64_t ldp, float scaling,
                                                               bf16_t* __restrict__ dlogits, int64_t ldd) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        const float sr = s[t];
        float pv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) pv[h] = lane + 64 * h < E ? bf2f(p[t * ldp + lane + 64 * h]) : 0.f;
        int ex[MOE_MAX_K];
        float g[MOE_MAX_K];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                const int e = idx[t * k + j];
                const bool ok = e >= 0 && e < E;
                const float lo = __shfl(pv[0], ok ? (e & 63) : 0, 64), hi = __shfl(pv[1], ok ? (e & 63) : 0, 64);
                ex[j] = e;
                g[j] = dw[t * k + j];
                dot += g[j] * (ok ? (e >= 64 ? hi : lo) : 0.f);  // slot order
            }
        dot /= sr;
        float gp[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                const float dv = scaling * (g[j] - dot) / sr;
                if (ex[j] == lane) gp[0] += dv;
                if (ex[j] == lane + 64) gp[1] += dv;
            }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (lane + 64 * h < E) dlogits[t * ldd + lane + 64 * h] = f2bf(gp[h] * pv[h] * (1.0f - pv[h]));
    }
}

// ------------------------------------------------------------------------------------------------ squared-ReLU GLU
// A thread moves 16 bytes; c8 = F / 8 pieces per row of a, twice that per row of [u | g].  Rows the caller never filled (the sorted buffer's padding) may
// hold anything: every access stays inside the row it belongs to.
__global__ __launch_bounds__(256) void latmoe_relu2_glu_fwd_kernel(int64_t R, int c8, const bf16_t* __restrict__ gu, int64_t ldg, bf16_t* __restrict__ a, int64_t lda) {
    const int64_t n = R * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / c8;
        const int c = (int)(i - r * c8);
        float u[8], g[8], o[8];
        unpack8(*(const u32x4*)(gu + r * ldg + c * 8), u);
        unpack8(*(const u32x4*)(gu + r * ldg + (int64_t)(c8 + c) * 8), g);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float rl = g[q] > 0.f ? g[q] : 0.f;
            o[q] = u[q] * rbf(rl * rl);
        }
        *(u32x4*)(a + r * lda + c * 8) = pack8(o);
    }
}

// du = bf16(da * q), q = bf16(relu(g)^2);  dg = bf16(da * u * 2 relu(g)), exactly zero where g <= 0
__global__ __launch_bounds__(256) void latmoe_relu2_glu_bwd_kernel(int64_t R, int c8, const bf16_t* __restrict__ gu, int64_t ldg, const bf16_t* __restrict__ da,
                                                                   int64_t ldda, bf16_t* __restrict__ dgu, int64_t lddg) {
    const int64_t n = R * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / c8;
        const int c = (int)(i - r * c8);
        float u[8], g[8], d[8], du[8], dg[8];
        unpack8(*(const u32x4*)(gu + r * ldg + c * 8), u);
        unpack8(*(const u32x4*)(gu + r * ldg + (int64_t)(c8 + c) * 8), g);
        unpack8(*(const u32x4*)(da + r * ldda + c * 8), d);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool on = g[q] > 0.f;
            du[q] = on ? d[q] * rbf(g[q] * g[q]) : 0.f;
            dg[q] = on ? d[q] * u[q] * (2.0f * g[q]) : 0.f;
        }
        *(u32x4*)(dgu + r * lddg + c * 8) = pack8(du);
        *(u32x4*)(dgu + r * lddg + (int64_t)(c8 + c) * 8) = pack8(dg);
    }
}

}  // namespace

extern "C" int mi355_latmoe_route_fwd(int64_t T, int E, int k, const void* logits, int64_t ldl, const void* biases, int bias_dtype, const int32_t* forced_idx,
                                      float scaling, void* p, int64_t ldp, int32_t* idx, void* w, float* s, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_latmoe_route_fwd", T, E, k)) return 1;
    MI355_REQUIRE(logits && p && idx && w && s, "mi355_latmoe_route_fwd: null pointer");
    MI355_REQUIRE(forced_idx || biases, "mi355_latmoe_route_fwd: the selection needs the balancing biases unless it is forced");
    MI355_REQUIRE(forced_idx || bias_dtype_ok(bias_dtype), "mi355_latmoe_route_fwd: the biases are bf16 or fp32 (got dtype code %d)", bias_dtype);
    MI355_REQUIRE(ldl >= E && ldp >= E, "mi355_latmoe_route_fwd: a leading dimension is below the routed experts = %d", E);
    const int grid = capped_grid((T + 3) / 4);
    const bf16_t* lg = (const bf16_t*)logits;
    if (forced_idx)
        latmoe_route_fwd_kernel<false, true><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, nullptr, forced_idx, scaling, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    else if (bias_dtype == MI355_DT_F32)
        latmoe_route_fwd_kernel<true, false><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, biases, nullptr, scaling, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    else
        latmoe_route_fwd_kernel<false, false><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, biases, nullptr, scaling, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    MI355_LAUNCH_CHECK("mi355_latmoe_route_fwd");
    return 0;
}

extern "C" int mi355_latmoe_route_bwd(int64_t T, int E, int k, const float* dw, const float* s, const int32_t* idx, const void* p, int64_t ldp, float scaling,
                                      void* dlogits, int64_t ldd, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_latmoe_route_bwd", T, E, k)) return 1;
    MI355_REQUIRE(dw && s && idx && p && dlogits, "mi355_latmoe_route_bwd: null pointer");
    MI355_REQUIRE(ldp >= E && ldd >= E, "mi355_latmoe_route_bwd: a leading dimension is below the routed experts = %d", E);
    latmoe_route_bwd_kernel<<<capped_grid((T + 3) / 4), 256, 0, ST(stream)>>>(T, E, k, dw, s, idx, (const bf16_t*)p, ldp, scaling, (bf16_t*)dlogits, ldd);
    MI355_LAUNCH_CHECK("mi355_latmoe_route_bwd");
    return 0;
}

extern "C" int mi355_latmoe_relu2_glu_fwd(int64_t R, int F, const void* gu, int64_t ldg, void* a, int64_t lda, void* stream) {
    if (R <= 0) return 0;
    MI355_REQUIRE(F > 0 && F <= (1 << 29), "mi355_latmoe_relu2_glu_fwd: the hidden size must be in 1..2^29 (got %d)", F);
    if (check_rows("mi355_latmoe_relu2_glu_fwd", R, F, {lda}) || check_rows("mi355_latmoe_relu2_glu_fwd", R, 2 * F, {ldg})) return 1;
    MI355_REQUIRE(gu && a, "mi355_latmoe_relu2_glu_fwd: null pointer");
    MI355_REQUIRE(aligned16({gu, a}), "mi355_latmoe_relu2_glu_fwd: the rows must be 16-byte aligned");
    latmoe_relu2_glu_fwd_kernel<<<capped_grid((R * (F >> 3) + 255) / 256), 256, 0, ST(stream)>>>(R, F >> 3, (const bf16_t*)gu, ldg, (bf16_t*)a, lda);
    MI355_LAUNCH_CHECK("mi355_latmoe_relu2_glu_fwd");
    return 0;
}

extern "C" int mi355_latmoe_relu2_glu_bwd(int64_t R, int F, const void* gu, int64_t ldg, const void* da, int64_t ldda, void* dgu, int64_t lddg, void* stream) {
    if (R <= 0) return 0;
    MI355_REQUIRE(F > 0 && F <= (1 << 29), "mi355_latmoe_relu2_glu_bwd: the hidden size must be in 1..2^29 (got %d)", F);
    if (check_rows("mi355_latmoe_relu2_glu_bwd", R, F, {ldda}) || check_rows("mi355_latmoe_relu2_glu_bwd", R, 2 * F, {ldg, lddg})) return 1;
    MI355_REQUIRE(gu && da && dgu, "mi355_latmoe_relu2_glu_bwd: null pointer");
    MI355_REQUIRE(aligned16({gu, da, dgu}), "mi355_latmoe_relu2_glu_bwd: the rows must be 16-byte aligned");
    latmoe_relu2_glu_bwd_kernel<<<capped_grid((R * (F >> 3) + 255) / 256), 256, 0, ST(stream)>>>(R, F >> 3, (const bf16_t*)gu, ldg, (const bf16_t*)da, ldda, (bf16_t*)dgu,
                                                                                                    lddg);
    MI355_LAUNCH_CHECK("mi355_latmoe_relu2_glu_bwd");
    return 0;
}
