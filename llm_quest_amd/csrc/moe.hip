// Qwen3 mixture-of-experts (reference llm_quest/moe/qwen3_moe.py:104-167): everything of Qwen3MoE.forward that is not a matrix product.
//
//   route     softmax over the E gate logits of a token, the k largest probabilities (ties: the lower expert index), their renormalised weights
//   plan      the stable counting sort of the T * k assignments by expert: counts, segment offsets (each start a multiple of MOE_ALIGN rows),
//             slot[t, j] = the row of assignment (t, j) in the expert-sorted buffer, row_token[r] = its inverse (-1 on padding rows), and the
//             load-balancing loss from the counts and the column sums of the probabilities
//   gather    Xs[r] = x[row_token[r]]                                (padding rows zero)
//   combine   out[t] = residual[t] + (shared[t] + sum_j w[t, j] * Y[slot[t, j]])   (j ascending, fp32, one rounding) -- also the gather's backward with w = NULL;
//             the ONE combine kernel and its launcher: mi355_dsmoe_combine_fwd (deepseek_moe.hip) supplies ``shared``, mi355_moe_combine_fwd passes none
//   and the backwards of combine and route.
//
// The expert products themselves run as segmented GEMMs (gemm_segmented.hip: mi355_gemm_bf16_segmented / _segmented_tn), one launch per product over all experts, on the
// row segments this plan leaves in device memory (counts, offsets); nothing here is read back by the host.
//
// No atomics and no workgroup that waits for another: the sort is three launches (per-chunk ranks and histograms, ONE workgroup for the scan over
// chunks and experts, the scatter), every output element has exactly one writer, every sum a fixed order -- two runs give the same bits.
// Rows move 16 bytes per lane; sums are fp32 and are rounded to bf16 exactly where the reference's bf16 tensors are:
//   p = bf16(softmax), s = bf16(sum_j v_j), w_j = bf16(v_j / s)      (qwen3_moe.py:113-121)
// The limits, the host checks and the two ends of the router kernel that deepseek_moe.hip uses as well are moe_common.h.
#include "moe_common.h"

namespace {

constexpr int MOE_ALIGN = 32;     // rows: every expert's segment starts at a multiple of this
constexpr int PLAN_CHUNK = 2048;  // assignments per workgroup of the counting pass

// bf16 bits -> an unsigned short that orders like the value (negative values below positive ones)
__device__ __forceinline__ unsigned order_bits(bf16_t b) { return (b & 0x8000u) ? (~(unsigned)b & 0xffffu) : ((unsigned)b | 0x8000u); }
__device__ __forceinline__ bf16_t unorder_bits(unsigned o) { return (bf16_t)((o & 0x8000u) ? (o & 0x7fffu) : (~o & 0xffffu)); }

// ------------------------------------------------------------------------------------------------ route, forward
// One wave per token; lane l holds experts l and l + 64.  The selection key is (ordered bf16 bits << 8) | (255 - expert): the wave maximum is the
// largest probability, and among equal ones the lowest expert.  A taken expert's key becomes 0 (a live key is at least 255 - 127).
template <bool REPLAY>
__global__ __launch_bounds__(256) void moe_route_fwd_kernel(int64_t T, int E, int k, const bf16_t* __restrict__ in, int64_t ldin, bf16_t* __restrict__ p,
                                                            int64_t ldp, int* __restrict__ idx, bf16_t* __restrict__ w, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        const bf16_t* row = in + t * ldin;
        bf16_t pb[2];
        if (REPLAY) {
#pragma unroll
            for (int h = 0; h < 2; ++h) pb[h] = lane + 64 * h < E ? row[lane + 64 * h] : (bf16_t)0;
        } else {
            route_softmax(row, E, lane, pb);
        }
        if (p != nullptr) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (lane + 64 * h < E) p[t * ldp + lane + 64 * h] = pb[h];
        }
        unsigned key[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) key[h] = lane + 64 * h < E ? (order_bits(pb[h]) << 8) | (unsigned)(255 - (lane + 64 * h)) : 0u;
        float v[MOE_MAX_K];
        int ex[MOE_MAX_K];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j) {
            if (j < k) {
                const unsigned best = wave_umax(key[0] > key[1] ? key[0] : key[1]);
                ex[j] = 255 - (int)(best & 0xffu);
                v[j] = bf2f(unorder_bits(best >> 8));
                sum += v[j];  // slot order
                if (key[0] == best) key[0] = 0u;
                if (key[1] == best) key[1] = 0u;
            }
        }
        route_write(t, k, lane, ex, v, sum, idx, w, s);
    }
}

// ------------------------------------------------------------------------------------------------ route, backward
// gv_j = (dw_j - sum_m dw_m w_m) / s;  gp_e = [e selected as j] gv_j + g coef E f_e / T;  dlogits_e = bf16(p_e (gp_e - sum_e' p_e' gp_e')).
__global__ __launch_bounds__(256) void moe_route_bwd_kernel(int64_t T, int E, int k, const float* __restrict__ dw, const bf16_t* __restrict__ w,
                                                            const float* __restrict__ s, const int* __restrict__ idx, const bf16_t* __restrict__ p,
                                                            int64_t ldp, const int* __restrict__ counts, const float* __restrict__ g, float coef,
                                                            bf16_t* __restrict__ dlogits, int64_t ldd) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    const float gl = g != nullptr ? g[0] * coef * (float)E / (float)T : 0.f;
    float aux[2];  // the load loss's share of gp: f carries no gradient, P = mean_t p does
#pragma unroll
    for (int h = 0; h < 2; ++h) aux[h] = (g != nullptr && lane + 64 * h < E) ? gl * ((float)counts[lane + 64 * h] / ((float)k * (float)T)) : 0.f;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += waves) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < MOE_MAX_K; ++j)
            if (j < k) dot += dw[t * k + j] * bf2f(w[t * k + j]);
        const float sr = s[t];
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
            if (lane + 64 * h < E) dlogits[t * ldd + lane + 64 * h] = f2bf(pv[h] * (gp[h] - mean));
    }
}

// ------------------------------------------------------------------------------------------------ plan
// Pass 1: a workgroup takes PLAN_CHUNK consecutive assignments (i = t * k + j order).  Thread e walks the chunk in that order and hands every
// assignment of expert e its rank inside the chunk (parked in slot[i]: each i has one expert, so one writer), and leaves the chunk's count.
__global__ __launch_bounds__(128) void moe_plan_count_kernel(int64_t n, int E, const int* __restrict__ idx, int* __restrict__ slot, int* __restrict__ hist) {
    __shared__ int ids[PLAN_CHUNK];
    const int64_t i0 = (int64_t)blockIdx.x * PLAN_CHUNK;
    const int len = (int)(n - i0 < PLAN_CHUNK ? n - i0 : PLAN_CHUNK);
    for (int i = threadIdx.x; i < len; i += 128) ids[i] = idx[i0 + i];
    __syncthreads();
    const int e = threadIdx.x;
    if (e < E) {
        int c = 0;
        for (int i = 0; i < len; ++i)
            if (ids[i] == e) slot[i0 + i] = c++;
        hist[(int64_t)blockIdx.x * E + e] = c;
    }
}

// Pass 2, ONE workgroup: thread e turns the chunk counts of expert e into running bases (exclusive scan over chunks, in place) and the total;
// thread 0 then lays the segments out, every start rounded up to MOE_ALIGN, and finishes the load loss
//   loss = coef * E * sum_e f_e P_e,  f_e = counts_e / (k T),  P_e = psum_e / T    (qwen3_moe.py:124-129), fp32.
__global__ __launch_bounds__(128) void moe_plan_scan_kernel(int64_t T, int E, int k, int64_t chunks, int* __restrict__ hist, int* __restrict__ counts,
                                                            int* __restrict__ offsets, const float* __restrict__ psum, float coef, float* __restrict__ loss) {
    __shared__ int tot[MOE_MAX_E];
    const int e = threadIdx.x;
    if (e < E) {
        int run = 0;
        for (int64_t b = 0; b < chunks; ++b) {
            const int c = hist[b * E + e];
            hist[b * E + e] = run;
            run += c;
        }
        tot[e] = run;
        counts[e] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0;
        float acc = 0.f;
        for (int x = 0; x < E; ++x) {
            offsets[x] = off;
            off += (tot[x] + MOE_ALIGN - 1) / MOE_ALIGN * MOE_ALIGN;
            if (psum != nullptr) acc += ((float)tot[x] / ((float)k * (float)T)) * (psum[x] / (float)T);
        }
        offsets[E] = off;
        if (psum != nullptr && loss != nullptr) loss[0] = coef * (float)E * acc;
    }
}

// Pass 3: slot = segment start + chunk base + rank in the chunk; the inverse map.  row_token was filled with -1 before.
__global__ __launch_bounds__(256) void moe_plan_scatter_kernel(int64_t n, int E, int k, int64_t R, const int* __restrict__ idx, const int* __restrict__ hist,
                                                               const int* __restrict__ offsets, int* __restrict__ slot, int* __restrict__ row_token) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int e = idx[i];
        if (e < 0 || e >= E) {  // not an expert: the assignment gets no row (the combine kernels skip a negative slot)
            slot[i] = -1;
            continue;
        }
        const int64_t r = (int64_t)offsets[e] + hist[(i / PLAN_CHUNK) * E + e] + slot[i];
        slot[i] = (int)r;
        if (r < R) row_token[r] = (int)(i / k);
    }
}

// ------------------------------------------------------------------------------------------------ rows
// A thread moves 16 bytes; c8 = d / 8 pieces per row.
__global__ __launch_bounds__(256) void moe_gather_kernel(int64_t R, int64_t T, int c8, const int* __restrict__ row_token, const bf16_t* __restrict__ x,
                                                         int64_t ldx, bf16_t* __restrict__ xs, int64_t ldxs) {
    const int64_t n = R * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t r = i / c8;
        const int c = (int)(i - r * c8);
        const int t = row_token[r];
        u32x4 v = {0u, 0u, 0u, 0u};
        if (t >= 0 && t < T) v = *(const u32x4*)(x + (int64_t)t * ldx + c * 8);
        *(u32x4*)(xs + r * ldxs + c * 8) = v;
    }
}

// out[t] = res[t] + (sh[t] + sum_j w[t, j] * Y[slot[t, j]]); w (weights of 1), sh and res may each be null -- both combine entry points launch this kernel
__global__ __launch_bounds__(256) void moe_combine_fwd_kernel(int64_t T, int64_t R, int k, int c8, const int* __restrict__ slot, const bf16_t* __restrict__ w,
                                                              const bf16_t* __restrict__ y, int64_t ldy, const bf16_t* __restrict__ sh, int64_t lds,
                                                              const bf16_t* __restrict__ res, int64_t ldr, bf16_t* __restrict__ out, int64_t ldo) {
    const int64_t n = T * c8, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int64_t t = i / c8;
        const int c = (int)(i - t * c8);
        float acc[8], f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int j = 0; j < k; ++j) {
            const int r = slot[t * k + j];
            if (r < 0 || r >= R) continue;
            const float wj = w != nullptr ? bf2f(w[t * k + j]) : 1.f;
            unpack8(*(const u32x4*)(y + (int64_t)r * ldy + c * 8), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += wj * f[e];
        }
        if (sh != nullptr) {
            unpack8(*(const u32x4*)(sh + t * lds + c * 8), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = f[e] + acc[e];
        }
        if (res != nullptr) {
            unpack8(*(const u32x4*)(res + t * ldr + c * 8), f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = f[e] + acc[e];
        }
        *(u32x4*)(out + t * ldo + c * 8) = pack8(acc);
    }
}

// One wave per sorted row r: dY[r] = bf16(w(r) * dout[token(r)]) and dw[t, j] = <dout[t], Y[r]> for the one (t, j) with slot[t, j] = r.
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(int64_t T, int64_t R, int k, int c8, const int* __restrict__ row_token, const int* __restrict__ slot,
                                                              const bf16_t* __restrict__ w, const bf16_t* __restrict__ dout, int64_t ldd,
                                                              const bf16_t* __restrict__ y, int64_t ldy, bf16_t* __restrict__ dy, int64_t lddy,
                                                              float* __restrict__ dw) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < R; r += waves) {
        const int t = row_token[r];
        int j = -1;
        if (t >= 0 && t < T)
            for (int q = 0; q < k; ++q)
                if (slot[(int64_t)t * k + q] == r) j = q;
        if (j < 0) {
            const u32x4 z = {0u, 0u, 0u, 0u};
            for (int c = lane; c < c8; c += 64) *(u32x4*)(dy + r * lddy + c * 8) = z;
            continue;
        }
        const float wj = w != nullptr ? bf2f(w[(int64_t)t * k + j]) : 1.f;
        float dot = 0.f;
        for (int c = lane; c < c8; c += 64) {
            float d[8], f[8], o[8];
            unpack8(*(const u32x4*)(dout + (int64_t)t * ldd + c * 8), d);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = wj * d[e];
            *(u32x4*)(dy + r * lddy + c * 8) = pack8(o);
            if (dw != nullptr) {
                unpack8(*(const u32x4*)(y + r * ldy + c * 8), f);
#pragma unroll
                for (int e = 0; e < 8; ++e) dot += d[e] * f[e];
            }
        }
        if (dw != nullptr) {
            dot = wave_sum(dot);
            if (lane == 0) dw[(int64_t)t * k + j] = dot;
        }
    }
}

int64_t plan_chunks(int64_t T, int k) { return (T * k + PLAN_CHUNK - 1) / PLAN_CHUNK; }

}  // namespace

extern "C" int mi355_moe_row_align(void) { return MOE_ALIGN; }

extern "C" int64_t mi355_moe_plan_workspace_bytes(int64_t T, int E, int k) {
    if (T <= 0 || E <= 0 || E > MOE_MAX_E || k <= 0 || k > MOE_MAX_K || T >= (int64_t)1 << 31) return 0;
    return plan_chunks(T, k) * E * (int64_t)sizeof(int);
}

extern "C" int mi355_moe_route_fwd(int64_t T, int E, int k, const void* in, int64_t ldin, int replay, void* p, int64_t ldp, int32_t* idx, void* w, float* s,
                                   void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_moe_route_fwd", T, E, k)) return 1;
    MI355_REQUIRE(in && idx && w && s, "mi355_moe_route_fwd: null pointer");
    MI355_REQUIRE(replay || p, "mi355_moe_route_fwd: the probabilities need a destination unless they are replayed");
    MI355_REQUIRE(ldin >= E && (!p || ldp >= E), "mi355_moe_route_fwd: a leading dimension is below num_experts = %d", E);
    const int grid = capped_grid((T + 3) / 4);
    if (replay)
        moe_route_fwd_kernel<true><<<grid, 256, 0, ST(stream)>>>(T, E, k, (const bf16_t*)in, ldin, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    else
        moe_route_fwd_kernel<false><<<grid, 256, 0, ST(stream)>>>(T, E, k, (const bf16_t*)in, ldin, (bf16_t*)p, ldp, idx, (bf16_t*)w, s);
    MI355_LAUNCH_CHECK("mi355_moe_route_fwd");
    return 0;
}

extern "C" int mi355_moe_route_bwd(int64_t T, int E, int k, const float* dw, const void* w, const float* s, const int32_t* idx, const void* p, int64_t ldp,
                                   const int32_t* counts, const float* g, float aux_loss_coef, void* dlogits, int64_t ldd, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_moe_route_bwd", T, E, k)) return 1;
    MI355_REQUIRE(dw && w && s && idx && p && dlogits, "mi355_moe_route_bwd: null pointer");
    MI355_REQUIRE(!g || counts, "mi355_moe_route_bwd: the load loss's gradient needs the counts");
    MI355_REQUIRE(ldp >= E && ldd >= E, "mi355_moe_route_bwd: a leading dimension is below num_experts = %d", E);
    moe_route_bwd_kernel<<<capped_grid((T + 3) / 4), 256, 0, ST(stream)>>>(T, E, k, dw, (const bf16_t*)w, s, idx, (const bf16_t*)p, ldp, counts, g, aux_loss_coef,
                                                                             (bf16_t*)dlogits, ldd);
    MI355_LAUNCH_CHECK("mi355_moe_route_bwd");
    return 0;
}

extern "C" int mi355_moe_plan(int64_t T, int E, int k, const int32_t* idx, int32_t* counts, int32_t* offsets, int32_t* slot, int32_t* row_token, int64_t R,
                              const float* psum, float aux_loss_coef, float* loss, void* workspace, int64_t workspace_bytes, void* stream) {
    if (T <= 0) return 0;
    if (check_route("mi355_moe_plan", T, E, k)) return 1;
    MI355_REQUIRE(idx && counts && offsets && slot && row_token && workspace, "mi355_moe_plan: null pointer");
    MI355_REQUIRE(!psum || loss, "mi355_moe_plan: the load loss needs a destination");
    MI355_REQUIRE(R >= T * k + (int64_t)E * (MOE_ALIGN - 1) && R < (int64_t)1 << 31,
                  "mi355_moe_plan: the sorted buffer needs tokens * top_k + num_experts * %d = %ld rows (got %ld)", MOE_ALIGN - 1, (long)(T * k + (int64_t)E * (MOE_ALIGN - 1)),
                  (long)R);
    const int64_t chunks = plan_chunks(T, k);
    MI355_REQUIRE(workspace_bytes >= chunks * E * (int64_t)sizeof(int) && ((uintptr_t)workspace & 3) == 0,
                  "mi355_moe_plan: workspace of %ld bytes needed (mi355_moe_plan_workspace_bytes), 4-byte aligned", (long)(chunks * E * (int64_t)sizeof(int)));
    const int64_t n = T * k;
    hipStream_t st = ST(stream);
    if (hipMemsetAsync(row_token, 0xff, (size_t)R * sizeof(int), st) != hipSuccess) {  // -1 everywhere; the scatter pass overwrites the rows in use
        mi355_set_error("mi355_moe_plan: memset failed");
        return 2;
    }
    moe_plan_count_kernel<<<(unsigned)chunks, 128, 0, st>>>(n, E, idx, slot, (int*)workspace);
    MI355_LAUNCH_CHECK("mi355_moe_plan(count)");
    moe_plan_scan_kernel<<<1, 128, 0, st>>>(T, E, k, chunks, (int*)workspace, counts, offsets, psum, aux_loss_coef, loss);
    MI355_LAUNCH_CHECK("mi355_moe_plan(scan)");
    moe_plan_scatter_kernel<<<capped_grid((n + 255) / 256), 256, 0, st>>>(n, E, k, R, idx, (const int*)workspace, offsets, slot, row_token);
    MI355_LAUNCH_CHECK("mi355_moe_plan(scatter)");
    return 0;
}

extern "C" int mi355_moe_gather_rows(int64_t R, int64_t T, int d, const int32_t* row_token, const void* x, int64_t ldx, void* xs, int64_t ldxs, void* stream) {
    if (R <= 0 || T <= 0) return 0;
    if (check_rows("mi355_moe_gather_rows", T, d, {ldx}) || check_rows("mi355_moe_gather_rows", R, d, {ldxs})) return 1;
    MI355_REQUIRE(row_token && x && xs, "mi355_moe_gather_rows: null pointer");
    MI355_REQUIRE(aligned16({x, xs}), "mi355_moe_gather_rows: x and xs must be 16-byte aligned");
    moe_gather_kernel<<<capped_grid((R * (d >> 3) + 255) / 256), 256, 0, ST(stream)>>>(R, T, d >> 3, row_token, (const bf16_t*)x, ldx, (bf16_t*)xs, ldxs);
    MI355_LAUNCH_CHECK("mi355_moe_gather_rows");
    return 0;
}

// The one combine launcher (declared in moe_common.h): mi355_moe_combine_fwd and mi355_dsmoe_combine_fwd are this call under their own name.
int moe_combine_fwd_launch(const char* who, int64_t T, int64_t R, int k, int d, const int32_t* slot, const void* w, const void* y, int64_t ldy, const void* shared,
                           int64_t lds, const void* residual, int64_t ldr, void* out, int64_t ldo, void* stream) {
    if (T <= 0) return 0;
    MI355_REQUIRE(k >= 1 && k <= MOE_MAX_K, "%s: top_k must be in 1..%d (got %d)", who, MOE_MAX_K, k);
    if (check_rows(who, T, d, {ldo}) || check_rows(who, R, d, {ldy})) return 1;
    if (shared && check_rows(who, T, d, {lds})) return 1;
    if (residual && check_rows(who, T, d, {ldr})) return 1;
    MI355_REQUIRE(R > 0, "%s: the sorted rows must be positive (got %ld)", who, (long)R);
    MI355_REQUIRE(slot && y && out, "%s: null pointer", who);
    MI355_REQUIRE(aligned16({y, shared, residual, out}), "%s: y, shared, residual and out must be 16-byte aligned", who);
    moe_combine_fwd_kernel<<<capped_grid((T * (d >> 3) + 255) / 256), 256, 0, ST(stream)>>>(T, R, k, d >> 3, slot, (const bf16_t*)w, (const bf16_t*)y, ldy,
                                                                                               (const bf16_t*)shared, lds, (const bf16_t*)residual, ldr, (bf16_t*)out, ldo);
    MI355_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int mi355_moe_combine_fwd(int64_t T, int64_t R, int k, int d, const int32_t* slot, const void* w, const void* y, int64_t ldy, const void* residual,
                                     int64_t ldr, void* out, int64_t ldo, void* stream) {
    return moe_combine_fwd_launch("mi355_moe_combine_fwd", T, R, k, d, slot, w, y, ldy, nullptr, 0, residual, ldr, out, ldo, stream);
}

extern "C" int mi355_moe_combine_bwd(int64_t T, int64_t R, int k, int d, const int32_t* row_token, const int32_t* slot, const void* w, const void* dout, int64_t ldd,
                                     const void* y, int64_t ldy, void* dy, int64_t lddy, float* dw, void* stream) {
    if (T <= 0 || R <= 0) return 0;
    MI355_REQUIRE(k >= 1 && k <= MOE_MAX_K, "mi355_moe_combine_bwd: top_k must be in 1..%d (got %d)", MOE_MAX_K, k);
    if (check_rows("mi355_moe_combine_bwd", T, d, {ldd}) || check_rows("mi355_moe_combine_bwd", R, d, {lddy})) return 1;
    if (dw && check_rows("mi355_moe_combine_bwd", R, d, {ldy})) return 1;
    MI355_REQUIRE(row_token && slot && dout && dy && (!dw || y), "mi355_moe_combine_bwd: null pointer");
    MI355_REQUIRE(aligned16({dout, y, dy}), "mi355_moe_combine_bwd: dout, y and dy must be 16-byte aligned");
    moe_combine_bwd_kernel<<<capped_grid((R + 3) / 4), 256, 0, ST(stream)>>>(T, R, k, d >> 3, row_token, slot, (const bf16_t*)w, (const bf16_t*)dout, ldd,
                                                                               (const bf16_t*)y, ldy, (bf16_t*)dy, lddy, dw);
    MI355_LAUNCH_CHECK("mi355_moe_combine_bwd");
    return 0;
}
