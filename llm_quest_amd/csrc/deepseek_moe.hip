// DeepSeekMoE (reference llm_quest/moe/deepseek_moe.py:166-214): what the layer needs beyond the Qwen3 mixture-of-experts kernels of moe.hip.
//
//   route     softmax over the E gate logits of a token, selection of the k largest (probability + balancing bias) keys (ties: the lower expert
//             index), weights from the UNBIASED probabilities, renormalised; or, with a forced selection, the weights of the given experts
//   update    biases += rate * sign(mean(counts) - counts) and max_vio = (max(counts) - mean) / mean, from the counts mi355_moe_plan wrote
//   silu      the shared experts' bias + SiLU between their two products, forward and backward, over [T, n * hidden] rows
//   combine   out[t] = residual[t] + (shared[t] + sum_j w[t, j] * Y[slot[t, j]])   (fp32, one rounding): the entry point only; kernel and launcher are moe.hip's
//   colsum    column sums of bf16 rows as per-row-part partials in a fixed order (the bias gradients)
//
// The plan, the row dispatch, the combine's backward and the router's backward are moe.hip's (mi355_moe_route_bwd takes any E in 1..128); the limits, the
// host checks and the two ends of the router kernel (the token's softmax, the write-out of s / idx / w) are shared with it through moe_common.h, which also
// holds the bias-balanced selection between them (latent_moe.hip routes with it too).
// No atomics, one writer per element, fixed summation orders.  Rounding points are the reference's bf16 tensors:
//   p = bf16(softmax), key = p + biases in the promoted dtype, s = bf16(sum_j v_j), w_j = bf16(v_j / s)     (deepseek_moe.py:180-186)
//   pre = bf16(bf16(x W1) + b1), act = bf16(silu(pre))                                                        (deepseek_moe.py:82-88, 125-126)
#include "moe_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ route, forward
// One wave per token; lane l holds experts l and l + 64.  Columns at and beyond E are never read.
template <bool BIAS_F32, bool FORCED>
__global__ __launch_bounds__(256) void dsmoe_route_fwd_kernel(int64_t T, int E, int k, const bf16_t* __restrict__ logits, int64_t ldl, const void* __restrict__ bias,
                                                              const int* __restrict__ forced, bf16_t* __restrict__ p, int64_t ldp, int* __restrict__ idx,
                                                              bf16_t* __restrict__ w, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    float bv[2] = {0.f, 0.f};
    if (!FORCED) route_load_bias<BIAS_F32>(bias, E, lane, bv);
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        bf16_t pb[2];
        float pf[2];
        route_softmax(logits + t * ldl, E, lane, pb);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pf[h] = bf2f(pb[h]);
            if (lane + 64 * h < E) p[t * ldp + lane + 64 * h] = pb[h];
        }
        float v[MOE_MAX_K];
        int ex[MOE_MAX_K];
        const float sum = route_select_biased<BIAS_F32, FORCED>(pf, bv, FORCED ? forced + t * k : nullptr, E, k, lane, ex, v);  // moe_common.h
        route_write(t, k, lane, ex, v, sum, idx, w, s);
    }
}

// ------------------------------------------------------------------------------------------------ bias update + max violation
// ONE workgroup, thread e owns expert e: one writer per bias, the two reductions in LDS in a fixed order.
template <bool BIAS_F32>
__global__ __launch_bounds__(128) void dsmoe_bias_update_kernel(int E, const int* __restrict__ counts, void* __restrict__ biases, float rate, float* __restrict__ max_vio) {
    __shared__ int cs[MOE_MAX_E];
    __shared__ float stat[2];
    const int e = threadIdx.x;
    const int c = e < E ? counts[e] : 0;
    cs[e] = c;
    __syncthreads();
    if (e == 0) {
        long long tot = 0;
        int mx = 0;
        for (int i = 0; i < E; ++i) {
            tot += cs[i];
            mx = cs[i] > mx ? cs[i] : mx;
        }
        const float mean = (float)tot / (float)E;
        stat[0] = mean;
        if (max_vio != nullptr) max_vio[0] = ((float)mx - mean) / mean;
    }
    __syncthreads();
    if (e < E) {
        const float vio = stat[0] - (float)c;
        const float sg = vio > 0.f ? 1.f : (vio < 0.f ? -1.f : 0.f);
        if (BIAS_F32) {
            float* b = (float*)biases;
            b[e] = b[e] + rate * sg;
        } else {
            bf16_t* b = (bf16_t*)biases;
            b[e] = f2bf(bf2f(b[e]) + rate * sg);
        }
    }
}

// ------------------------------------------------------------------------------------------------ shared experts: bias + SiLU
// A thread moves 16 bytes; c8 = N / 8 pieces per row.  zp holds bf16(x W1) on entry and the pre-activation bf16(z + b) on exit.
__global__ __launch_bounds__(256) void dsmoe_bias_silu_fwd_kernel(int64_t T, int c8, bf16_t* __restrict__ zp, int64_t ldz, const bf16_t* __restrict__ bias,
                                                                  bf16_t* __restrict__ act, int64_t lda) {
    const int64_t n = T * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t t = i / c8;
        const int c = (int)(i - t * c8);
        float z[8], b[8], a[8];
        unpack8(*(const u32x4*)(zp + t * ldz + c * 8), z);
        unpack8(*(const u32x4*)(bias + c * 8), b);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            z[q] = rbf(z[q] + b[q]);
            a[q] = z[q] * sigmoid_fast(z[q]);
        }
        *(u32x4*)(zp + t * ldz + c * 8) = pack8(z);
        *(u32x4*)(act + t * lda + c * 8) = pack8(a);
    }
}

// dpre = bf16(da * silu'(pre)),  silu'(x) = sig(x) (1 + x (1 - sig(x)))
__global__ __launch_bounds__(256) void dsmoe_bias_silu_bwd_kernel(int64_t T, int c8, const bf16_t* __restrict__ pre, int64_t ldp, const bf16_t* __restrict__ da,
                                                                  int64_t ldda, bf16_t* __restrict__ dpre, int64_t lddp) {
    const int64_t n = T * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t t = i / c8;
        const int c = (int)(i - t * c8);
        float z[8], d[8], o[8];
        unpack8(*(const u32x4*)(pre + t * ldp + c * 8), z);
        unpack8(*(const u32x4*)(da + t * ldda + c * 8), d);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float sg = sigmoid_fast(z[q]);
            o[q] = d[q] * sg * (1.0f + z[q] * (1.0f - sg));
        }
        *(u32x4*)(dpre + t * lddp + c * 8) = pack8(o);
    }
}

// ------------------------------------------------------------------------------------------------ column sums in a fixed order (bias gradients)
// mi355_colsum folds its row blocks with fp32 atomics, whose order is not fixed.  Here workgroup (x, y) owns 512 columns of row part y: the four waves take rows
// r, r + 1, r + 2, r + 3, meet in LDS and write parts[y, column] -- one writer; mi355_reduce_rows_f32 folds the parts.
__global__ __launch_bounds__(256) void dsmoe_colsum_parts_kernel(int64_t T, int N, const bf16_t* __restrict__ x, int64_t ldx, float* __restrict__ parts, int64_t rows_per_part) {
    __shared__ float red[4][512];
    const int chunk = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 512 + chunk * 8;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_part;
    const int64_t r1 = r0 + rows_per_part < T ? r0 + rows_per_part : T;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (col < N) {  // N % 8 == 0: the whole piece is inside the row
        for (int64_t r = r0 + rl; r < r1; r += 4) {
            float f[8];
            unpack8(*(const u32x4*)(x + r * ldx + col), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += f[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][chunk * 8 + e] = s[e];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256) {
        const int gc = blockIdx.x * 512 + c;
        if (gc < N) parts[(int64_t)blockIdx.y * N + gc] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

}  // namespace

extern "C" int mi355_dsmoe_route_fwd(int64_t T, int E, int k, const void* logits, int64_t ldl, const void* biases, int bias_dtype, const int32_t* forced_idx,
                                     void* p, int64_t ldp, int32_t* idx, void* w, float* s, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_dsmoe_route_fwd", T, E, k)) return 1;
    MI355_REQUIRE(logits && p && idx && w && s, "mi355_dsmoe_route_fwd: null pointer");
    MI355_REQUIRE(forced_idx || biases, "mi355_dsmoe_route_fwd: the selection needs the balancing biases unless it is forced");
    MI355_REQUIRE(forced_idx || bias_dtype_ok(bias_dtype), "mi355_dsmoe_route_fwd: the biases are bf16 or fp32 (got dtype code %d)", bias_dtype);
    MI355_REQUIRE(ldl >= E && ldp >= E, "mi355_dsmoe_route_fwd: a leading dimension is below the routed experts = %d", E);
    const int grid = capped_grid((T + 3) / 4);
    const bf16_t* lg = (const bf16_t*)logits;
    if (forced_idx)
        dsmoe_route_fwd_kernel<false, true><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, nullptr, forced_idx, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    else if (bias_dtype == MI355_DT_F32)
        dsmoe_route_fwd_kernel<true, false><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, biases, nullptr, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    else
        dsmoe_route_fwd_kernel<false, false><<<grid, 256, 0, ST(stream)>>>(T, E, k, lg, ldl, biases, nullptr, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    MI355_LAUNCH_CHECK("mi355_dsmoe_route_fwd");
    return 0;
}

extern "C" int mi355_dsmoe_bias_update(int E, const int32_t* counts, void* biases, int bias_dtype, float rate, float* max_vio, void* stream) {
    MI355_REQUIRE(E >= 1 && E <= MOE_MAX_E, "mi355_dsmoe_bias_update: the number of routed experts must be in 1..%d (got %d)", MOE_MAX_E, E);
    MI355_REQUIRE(counts && biases, "mi355_dsmoe_bias_update: null pointer");
    MI355_REQUIRE(bias_dtype_ok(bias_dtype), "mi355_dsmoe_bias_update: the biases are bf16 or fp32 (got dtype code %d)", bias_dtype);
    if (bias_dtype == MI355_DT_F32)
        dsmoe_bias_update_kernel<true><<<1, 128, 0, ST(stream)>>>(E, counts, biases, rate, max_vio);
    else
        dsmoe_bias_update_kernel<false><<<1, 128, 0, ST(stream)>>>(E, counts, biases, rate, max_vio);
    MI355_LAUNCH_CHECK("mi355_dsmoe_bias_update");
    return 0;
}

extern "C" int mi355_dsmoe_bias_silu_fwd(int64_t T, int N, void* z_pre, int64_t ldz, const void* bias, void* act, int64_t lda, void* stream) {
    if (T <= 0) return 0;
    if (check_rows("mi355_dsmoe_bias_silu_fwd", T, N, {ldz, lda})) return 1;
    MI355_REQUIRE(z_pre && bias && act, "mi355_dsmoe_bias_silu_fwd: null pointer");
    MI355_REQUIRE(aligned16({z_pre, bias, act}), "mi355_dsmoe_bias_silu_fwd: the rows and the bias must be 16-byte aligned");
    dsmoe_bias_silu_fwd_kernel<<<capped_grid((T * (N >> 3) + 255) / 256), 256, 0, ST(stream)>>>(T, N >> 3, (bf16_t*)z_pre, ldz, (const bf16_t*)bias, (bf16_t*)act, lda);
    MI355_LAUNCH_CHECK("mi355_dsmoe_bias_silu_fwd");
    return 0;
}

extern "C" int mi355_dsmoe_bias_silu_bwd(int64_t T, int N, const void* pre, int64_t ldp, const void* dact, int64_t ldda, void* dpre, int64_t lddp, void* stream) {
    if (T <= 0) return 0;
    if (check_rows("mi355_dsmoe_bias_silu_bwd", T, N, {ldp, ldda, lddp})) return 1;
    MI355_REQUIRE(pre && dact && dpre, "mi355_dsmoe_bias_silu_bwd: null pointer");
    MI355_REQUIRE(aligned16({pre, dact, dpre}), "mi355_dsmoe_bias_silu_bwd: the rows must be 16-byte aligned");
    dsmoe_bias_silu_bwd_kernel<<<capped_grid((T * (N >> 3) + 255) / 256), 256, 0, ST(stream)>>>(T, N >> 3, (const bf16_t*)pre, ldp, (const bf16_t*)dact, ldda, (bf16_t*)dpre,
                                                                                                   lddp);
    MI355_LAUNCH_CHECK("mi355_dsmoe_bias_silu_bwd");
    return 0;
}

// The combine kernel and its launcher are moe.hip's; this entry point adds the shared operand and insists on the weights.
extern "C" int mi355_dsmoe_combine_fwd(int64_t T, int64_t R, int k, int d, const int32_t* slot, const void* w, const void* y, int64_t ldy, const void* shared, int64_t lds,
                                       const void* residual, int64_t ldr, void* out, int64_t ldo, void* stream) {
    if (T <= 0) return 0;
    MI355_REQUIRE(w, "mi355_dsmoe_combine_fwd: null pointer (the routed experts' weights)");
    return moe_combine_fwd_launch("mi355_dsmoe_combine_fwd", T, R, k, d, slot, w, y, ldy, shared, lds, residual, ldr, out, ldo, stream);
}

extern "C" int mi355_dsmoe_colsum_parts(int64_t T, int N, const void* x, int64_t ldx, float* parts, int n_parts, void* stream) {
    MI355_REQUIRE(T > 0, "mi355_dsmoe_colsum_parts: no rows (got %ld)", (long)T);
    if (check_rows("mi355_dsmoe_colsum_parts", T, N, {ldx})) return 1;
    MI355_REQUIRE(n_parts >= 1 && n_parts <= 1024, "mi355_dsmoe_colsum_parts: the number of row parts must be in 1..1024 (got %d)", n_parts);
    MI355_REQUIRE(x && parts, "mi355_dsmoe_colsum_parts: null pointer");
    MI355_REQUIRE(aligned16({x}), "mi355_dsmoe_colsum_parts: the rows must be 16-byte aligned");
    const int64_t rows_per_part = (T + n_parts - 1) / n_parts;
    dsmoe_colsum_parts_kernel<<<dim3((unsigned)((N + 511) / 512), (unsigned)n_parts), 256, 0, ST(stream)>>>(T, N, (const bf16_t*)x, ldx, parts, rows_per_part);
    MI355_LAUNCH_CHECK("mi355_dsmoe_colsum_parts");
    return 0;
}
