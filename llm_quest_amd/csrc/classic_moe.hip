// Classic mixture of experts (reference llm_quest/moe/classic_moe.py:19-125): what the layer needs beyond the kernels of moe.hip and deepseek_moe.hip.
//
//   route     softmax of the E gate logits of a token (the gate's bias already in), the k largest probabilities (ties: the lower expert index) or a forced
//             selection, their renormalised weights -- moe.hip's router -- and in the same pass the token's logsumexp for the router z-loss.  And its
//             backward: moe.hip's formula plus the z term.
//   loss      moe_loss = z_router_coeff * mean_t(lse_t^2) + the load loss mi355_moe_plan left: ONE workgroup, so the sum over tokens has one fixed order
//   bias_act  an expert's bias add (and erf GELU) on the expert-sorted buffer between / behind the two segmented products
//   colsum    the per-expert bias gradients: column sums over every expert's row segment
//
// The plan, the row dispatch, the combine and its backward are moe.hip's; the GELU backward is mi355_gelu_bwd (elementwise.hip) on the contiguous sorted
// buffer: the same rounding point, so no twin lives here.  Limits, host checks and the two ends of the router kernel are moe_common.h's.
// No atomics, one writer per element, fixed summation orders.  Rounding points are the reference's bf16 tensors:
//   p = bf16(softmax), s = bf16(sum_j v_j), w_j = bf16(v_j / s)                                 (classic_moe.py:84-86)
//   lse_t = bf16(m + log(sum_e exp(x_e - m))), m the row maximum;  q_t = bf16(lse_t^2);  zmean = bf16((sum_t q_t) / T), the sum in fp32: thread i adds
//   tokens i, i + 256, ... ascending, then a tree over the 256 threads;  moe_loss = bf16(bf16(z_router_coeff * zmean) + load)   (classic_moe.py:89, 96)
//   pre = bf16(z + b1), act = bf16(gelu_erf(pre));  y = bf16(z + b2)                            (classic_moe.py:24-26 on bf16 products)
//
// Which expert a sorted row belongs to is found by a search, not put on a grid dimension: the host may not read the counts, so a grid with the expert on one
// axis would need enough workgroups per expert for ALL rows (one expert may own them all), E times the work items for rows that mostly do not exist.
// Instead every workgroup keeps the segment table (offsets, counts: at most 2 * 128 ints) in LDS, a wave takes a row and finds, wave-uniformly and in at most
// 7 steps, the last expert whose segment starts at or before it; a row at or beyond that segment's end is padding and is skipped.  The column sums DO put the
// expert on the grid: their work per expert is a loop over its own rows, so an empty expert costs one idle workgroup and not a pass.
#include "moe_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ route, forward
// One wave per token; lane l holds experts l and l + 64.  Columns at and beyond E are never read.
template <bool FORCED>
__global__ __launch_bounds__(256) void cmoe_route_fwd_kernel(int64_t T, int E, int k, const bf16_t* __restrict__ logits, int64_t ldl, const int* __restrict__ forced,
                                                             bf16_t* __restrict__ p, int64_t ldp, int* __restrict__ idx, bf16_t* __restrict__ w,
                                                             float* __restrict__ s, float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    const float nobias[2] = {0.f, 0.f};
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        const bf16_t* row = logits + t * ldl;
        bf16_t pb[2];
        route_softmax(row, E, lane, pb);  // the probabilities are moe.hip's, bit for bit
        // the logsumexp with the row maximum subtracted: the same maximum and the same sum route_softmax forms
        float x[2], ex2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) x[h] = lane + 64 * h < E ? bf2f(row[lane + 64 * h]) : -INFINITY;
        const float m = wave_max(fmaxf(x[0], x[1]));
#pragma unroll
        for (int h = 0; h < 2; ++h) ex2[h] = lane + 64 * h < E ? expf(x[h] - m) : 0.f;
        const float den = wave_sum(ex2[0] + ex2[1]);
        if (lane == 0) lse[t] = rbf(m + logf(den));
        float pf[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pf[h] = 0.f;
            if (lane + 64 * h < E) {
                pf[h] = bf2f(pb[h]);
                p[t * ldp + lane + 64 * h] = pb[h];
            }
        }
        float v[MOE_MAX_K];
        int ex[MOE_MAX_K];
        // with biases of zero the key is bf16(p + 0) = p: the k largest bf16 probabilities, the lower expert first among equal ones (moe.hip's selection)
        const float sum = route_select_biased<false, FORCED>(pf, nobias, FORCED ? forced + t * k : nullptr, E, k, lane, ex, v);
        route_write(t, k, lane, ex, v, sum, idx, w, s);
    }
}

// ------------------------------------------------------------------------------------------------ route, backward
// gv_j = (dw_j - sum_m dw_m w_m) / s;  gp_e = [e selected as j] gv_j + g load_coeff E f_e / T;
// dlogits_e = bf16(p_e (gp_e - sum_e' p_e' gp_e') + g z_router_coeff 2 lse_t / T p_e): d(lse_t) / d(logits_e) = p_e, f carries no gradient.
__global__ __launch_bounds__(256) void cmoe_route_bwd_kernel(int64_t T, int E, int k, const float* __restrict__ dw, const bf16_t* __restrict__ w,
                                                             const float* __restrict__ s, const int* __restrict__ idx, const bf16_t* __restrict__ p, int64_t ldp,
                                                             const int* __restrict__ counts, const float* __restrict__ g, float load_coeff, float z_coeff,
                                                             const float* __restrict__ lse, bf16_t* __restrict__ dlogits, int64_t ldd) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    const float gl = g != nullptr ? g[0] * load_coeff * (float)E / (float)T : 0.f;
    const float gz = g != nullptr ? g[0] * z_coeff * 2.0f / (float)T : 0.f;
    float aux[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) aux[h] = (g != nullptr && lane + 64 * h < E) ? gl * ((float)counts[lane + 64 * h] / ((float)k * (float)T)) : 0.f;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) dot += dw[t * k + j] * bf2f(w[t * k + j]);
        const float sr = s[t];
        const float zt = g != nullptr ? gz * lse[t] : 0.f;
        float gp[2] = {aux[0], aux[1]}, pv[2];
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) {
                const int e = idx[t * k + j];
                const float gv = (dw[t * k + j] - dot) / sr;
                if (e == lane) gp[0] += gv;
                if (e == lane + 64) gp[1] += gv;
            }
#pragma unroll
        for (int h = 0; h < 2; ++h) pv[h] = lane + 64 * h < E ? bf2f(p[t * ldp + lane + 64 * h]) : 0.f;
        const float mean = wave_sum(pv[0] * gp[0] + pv[1] * gp[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (lane + 64 * h < E) dlogits[t * ldd + lane + 64 * h] = f2bf(pv[h] * (gp[h] - mean) + zt * pv[h]);
    }
}

// ------------------------------------------------------------------------------------------------ the loss
// ONE workgroup: thread i sums q_t = bf16(lse_t^2) over t = i, i + 256, ... ascending, a tree folds the 256 sums (strides 128, 64, ..., 1).
__global__ __launch_bounds__(256) void cmoe_loss_kernel(int64_t T, const float* __restrict__ lse, float z_coeff, const float* __restrict__ load, float* __restrict__ out) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t t = threadIdx.x; t < T; t += 256) {
        const float l = lse[t];
        acc += rbf(l * l);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float zmean = rbf(red[0] / (float)T);
        out[0] = rbf(rbf(z_coeff * zmean) + (load != nullptr ? load[0] : 0.f));
    }
}

// ------------------------------------------------------------------------------------------------ bias (+ GELU) on the sorted buffer
// the segment table in LDS; seg_of: the last expert whose segment starts at or before row r, or -1 when r lies behind that segment's end (padding)
struct SegTable {
    int off[MOE_MAX_E];
    int cnt[MOE_MAX_E];
};
__device__ __forceinline__ void seg_load(SegTable& tb, int E, const int* __restrict__ counts, const int* __restrict__ offsets) {
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        tb.off[e] = offsets[e];
        tb.cnt[e] = counts[e];
    }
    __syncthreads();
}
__device__ __forceinline__ int seg_of(const SegTable& tb, int E, int64_t r) {
    int lo = 0, hi = E - 1;  // invariant: the answer is in lo..hi (off[0] <= r is checked at the end)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)tb.off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    const int64_t start = tb.off[lo];
    return (r >= start && r < start + tb.cnt[lo]) ? lo : -1;
}

// One wave per sorted row, a lane moves 16 bytes.  GELU: pre = bf16(z + bias[e]) goes to ``pre`` (which may be z itself), act = bf16(gelu_erf(pre)) to ``act``;
// else only the sum goes to ``pre``.  Padding rows are neither read nor written.
template <bool GELU>
__global__ __launch_bounds__(256) void cmoe_bias_act_kernel(int64_t R, int c8, int E, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                            const bf16_t* z, int64_t ldz, const bf16_t* __restrict__ bias, int64_t stride_bias, bf16_t* pre,
                                                            int64_t ldp, bf16_t* __restrict__ act, int64_t lda) {  // pre may be z itself: no __restrict__ on the two
    __shared__ SegTable tb;
    seg_load(tb, E, counts, offsets);
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += waves) {
        const int e = seg_of(tb, E, r);
        if (e < 0) continue;
        const bf16_t* b = bias + (int64_t)e * stride_bias;
        for (int c = lane; c < c8; c += 64) {
            float v[8], bv[8];
            unpack8(*(const u32x4*)(z + r * ldz + c * 8), v);
            unpack8(*(const u32x4*)(b + c * 8), bv);
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = rbf(v[q] + bv[q]);
            *(u32x4*)(pre + r * ldp + c * 8) = pack8(v);
            if (GELU) {
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = gelu_val<0>(v[q]);
                *(u32x4*)(act + r * lda + c * 8) = pack8(v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ per-expert column sums
// Workgroup (x, e, y): 512 columns from 512 x, expert e, row part y of n_parts: rows offsets[e] + y * per .. + per of the segment, per = ceil(counts[e] / n_parts).
// 64 column pieces x 4 row lanes; a row lane adds its rows ascending (r, r + 4, ...), the four lanes fold as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(256) void cmoe_segsum_parts_kernel(int64_t R, int N, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                                const bf16_t* __restrict__ x, int64_t ldx, float* __restrict__ parts) {
    __shared__ float red[4][512];
    const int chunk = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int col = blockIdx.x * 512 + chunk * 8;
    const int e = blockIdx.y, n_parts = gridDim.z;
    const int64_t cnt = counts[e] > 0 ? counts[e] : 0, off = offsets[e] > 0 ? offsets[e] : 0;
    const int64_t per = (cnt + n_parts - 1) / n_parts;
    int64_t r0 = off + (int64_t)blockIdx.z * per, r1 = r0 + per;
    if (r1 > off + cnt) r1 = off + cnt;
    if (r1 > R) r1 = R;  // a table that points beyond the buffer reads nothing there
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (col < N) {  // N % 8 == 0: the whole piece is inside the row
        for (int64_t r = r0 + rl; r < r1; r += 4) {
            float f[8];
            unpack8(*(const u32x4*)(x + r * ldx + col), f);
#pragma unroll
            for (int q = 0; q < 8; ++q) s[q] += f[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) red[rl][chunk * 8 + q] = s[q];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256) {
        const int gc = blockIdx.x * 512 + c;
        if (gc < N) parts[((int64_t)e * n_parts + blockIdx.z) * N + gc] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// out[e, c] (+)= sum_y parts[e, y, c], y ascending.  Accumulating, an expert without a row is not touched (adding zero would turn a -0 into +0).
template <bool OUT_F32>
__global__ __launch_bounds__(256) void cmoe_segsum_fold_kernel(int E, int N, int n_parts, const int* __restrict__ counts, const float* __restrict__ parts,
                                                               void* __restrict__ out, int64_t stride_out, int accumulate) {
    const int64_t n = (int64_t)E * N, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int e = (int)(i / N);
        const int c = (int)(i - (int64_t)e * N);
        if (accumulate && counts[e] <= 0) continue;
        float acc = 0.f;
        for (int y = 0; y < n_parts; ++y) acc += parts[((int64_t)e * n_parts + y) * N + c];
        if (OUT_F32) {
            float* o = (float*)out + (int64_t)e * stride_out + c;
            *o = accumulate ? *o + acc : acc;
        } else {
            bf16_t* o = (bf16_t*)out + (int64_t)e * stride_out + c;
            *o = f2bf(accumulate ? bf2f(*o) + acc : acc);
        }
    }
}

inline int check_experts(const char* who, int E) {
    MI355_REQUIRE(E >= 1 && E <= MOE_MAX_E, "%s: num_experts must be in 1..%d (got %d)", who, MOE_MAX_E, E);
    return 0;
}

}  // namespace

extern "C" int mi355_cmoe_route_fwd(int64_t T, int E, int k, const void* logits, int64_t ldl, const int32_t* forced_idx, void* p, int64_t ldp, int32_t* idx, void* w,
                                    float* s, float* lse, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_cmoe_route_fwd", T, E, k)) return 1;
    MI355_REQUIRE(logits && p && idx && w && s && lse, "mi355_cmoe_route_fwd: null pointer");
    MI355_REQUIRE(ldl >= E && ldp >= E, "mi355_cmoe_route_fwd: a leading dimension is below num_experts = %d", E);
    const int grid = capped_grid((T + 3) / 4);
    if (forced_idx)
        cmoe_route_fwd_kernel<true><<<grid, 256, 0, ST(stream)>>>(T, E, k, (const bf16_t*)logits, ldl, forced_idx, (bf16_t*)p, ldp, idx, (bf16_t*)w, s, lse);
    else
        cmoe_route_fwd_kernel<false><<<grid, 256, 0, ST(stream)>>>(T, E, k, (const bf16_t*)logits, ldl, nullptr, (bf16_t*)p, ldp, idx, (bf16_t*)w, s, lse);
    MI355_LAUNCH_CHECK("mi355_cmoe_route_fwd");
    return 0;
}

extern "C" int mi355_cmoe_route_bwd(int64_t T, int E, int k, const float* dw, const void* w, const float* s, const int32_t* idx, const void* p, int64_t ldp,
                                    const int32_t* counts, const float* g, float load_coeff, float z_router_coeff, const float* lse, void* dlogits, int64_t ldd,
                                    void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_cmoe_route_bwd", T, E, k)) return 1;
    MI355_REQUIRE(dw && w && s && idx && p && dlogits, "mi355_cmoe_route_bwd: null pointer");
    MI355_REQUIRE(!g || (counts && lse), "mi355_cmoe_route_bwd: the loss's gradient needs the counts and the tokens' logsumexp");
    MI355_REQUIRE(ldp >= E && ldd >= E, "mi355_cmoe_route_bwd: a leading dimension is below num_experts = %d", E);
    cmoe_route_bwd_kernel<<<capped_grid((T + 3) / 4), 256, 0, ST(stream)>>>(T, E, k, dw, (const bf16_t*)w, s, idx, (const bf16_t*)p, ldp, counts, g, load_coeff,
                                                                              z_router_coeff, lse, (bf16_t*)dlogits, ldd);
    MI355_LAUNCH_CHECK("mi355_cmoe_route_bwd");
    return 0;
}

extern "C" int mi355_cmoe_loss(int64_t T, const float* lse, float z_router_coeff, const float* load_loss, float* moe_loss, void* stream) {
    if (T <= 0) return 0;
    MI355_REQUIRE(T < (int64_t)1 << 31, "mi355_cmoe_loss: tokens must stay below 2^31 (got %ld)", (long)T);
    MI355_REQUIRE(lse && moe_loss, "mi355_cmoe_loss: null pointer");
    cmoe_loss_kernel<<<1, 256, 0, ST(stream)>>>(T, lse, z_router_coeff, load_loss, moe_loss);
    MI355_LAUNCH_CHECK("mi355_cmoe_loss");
    return 0;
}

extern "C" int mi355_cmoe_bias_act_fwd(int64_t R, int N, int E, const int32_t* counts, const int32_t* offsets, void* z, int64_t ldz, const void* bias,
                                       int64_t stride_bias, void* pre, int64_t ldp, void* act, int64_t lda, int kind, void* stream) {
    if (R <= 0) return 0;
    MI355_REQUIRE(kind == 0 || kind == 1, "mi355_cmoe_bias_act_fwd: kind must be 0 (bias) or 1 (bias + GELU) (got %d)", kind);
    if (check_experts("mi355_cmoe_bias_act_fwd", E)) return 1;
    if (check_rows("mi355_cmoe_bias_act_fwd", R, N, {ldz})) return 1;
    if (pre && check_rows("mi355_cmoe_bias_act_fwd", R, N, {ldp})) return 1;
    if (kind == 1 && check_rows("mi355_cmoe_bias_act_fwd", R, N, {lda})) return 1;
    MI355_REQUIRE(counts && offsets && z && bias && (kind == 0 || act), "mi355_cmoe_bias_act_fwd: null pointer");
    MI355_REQUIRE(stride_bias >= 0 && (stride_bias & 7) == 0 && stride_bias < (int64_t)1 << 40,
                  "mi355_cmoe_bias_act_fwd: the distance between two experts' biases must be a non-negative multiple of 8 (got %ld)", (long)stride_bias);
    MI355_REQUIRE(aligned16({z, bias, pre, act}), "mi355_cmoe_bias_act_fwd: the rows and the biases must be 16-byte aligned");
    bf16_t* dst = pre ? (bf16_t*)pre : (bf16_t*)z;
    const int64_t ldd = pre ? ldp : ldz;
    const int grid = capped_grid((R + 3) / 4);
    if (kind == 1)
        cmoe_bias_act_kernel<true><<<grid, 256, 0, ST(stream)>>>(R, N >> 3, E, counts, offsets, (const bf16_t*)z, ldz, (const bf16_t*)bias, stride_bias, dst, ldd,
                                                                  (bf16_t*)act, lda);
    else
        cmoe_bias_act_kernel<false><<<grid, 256, 0, ST(stream)>>>(R, N >> 3, E, counts, offsets, (const bf16_t*)z, ldz, (const bf16_t*)bias, stride_bias, dst, ldd,
                                                                   nullptr, 0);
    MI355_LAUNCH_CHECK("mi355_cmoe_bias_act_fwd");
    return 0;
}

extern "C" int mi355_cmoe_segment_colsum(int64_t R, int N, int E, const int32_t* counts, const int32_t* offsets, const void* x, int64_t ldx, float* parts,
                                         int n_parts, void* out, int64_t stride_out, int out_dtype, int accumulate, void* stream) {
    if (R <= 0) return 0;
    if (check_experts("mi355_cmoe_segment_colsum", E)) return 1;
    if (check_rows("mi355_cmoe_segment_colsum", R, N, {ldx})) return 1;
    MI355_REQUIRE(n_parts >= 1 && n_parts <= 64, "mi355_cmoe_segment_colsum: the number of row parts must be in 1..64 (got %d)", n_parts);
    MI355_REQUIRE(bias_dtype_ok(out_dtype), "mi355_cmoe_segment_colsum: the sums are bf16 or fp32 (got dtype code %d)", out_dtype);
    MI355_REQUIRE(counts && offsets && x && parts && out, "mi355_cmoe_segment_colsum: null pointer");
    MI355_REQUIRE(stride_out >= N && stride_out < (int64_t)1 << 40, "mi355_cmoe_segment_colsum: the distance between two experts' sums must be at least the width %d (got %ld)", N,
                  (long)stride_out);
    MI355_REQUIRE(aligned16({x}) && ((uintptr_t)parts & 3) == 0, "mi355_cmoe_segment_colsum: the rows must be 16-byte aligned, the parts 4-byte aligned");
    cmoe_segsum_parts_kernel<<<dim3((unsigned)((N + 511) / 512), (unsigned)E, (unsigned)n_parts), 256, 0, ST(stream)>>>(R, N, counts, offsets, (const bf16_t*)x, ldx, parts);
    MI355_LAUNCH_CHECK("mi355_cmoe_segment_colsum(parts)");
    const int grid = capped_grid(((int64_t)E * N + 255) / 256);
    if (out_dtype == MI355_DT_F32)
        cmoe_segsum_fold_kernel<true><<<grid, 256, 0, ST(stream)>>>(E, N, n_parts, counts, parts, out, stride_out, accumulate);
    else
        cmoe_segsum_fold_kernel<false><<<grid, 256, 0, ST(stream)>>>(E, N, n_parts, counts, parts, out, stride_out, accumulate);
    MI355_LAUNCH_CHECK("mi355_cmoe_segment_colsum(fold)");
    return 0;
}
