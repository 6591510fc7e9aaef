// GRPO losses from hidden states (kernels_grpo_head.py): the row work between the GEMMs of a vocabulary-chunked LM head, so that the logits [B, S, V]
// never exist.  A chunk is bf16 [B S, Vc] at column offset c0 of the vocabulary (what one NT GEMM of the hidden states against rows [c0, c0 + Vc) of the
// head's weight writes).  Forward: an online log-sum-exp over the chunks, per-row state (m, l, label_logit) fp32 [B, S - 1], closed by the finish kernel.
// Backward: a recomputed chunk becomes its gradient g (onehot - exp(x - lse)) with the element formula of grpo.hip's label_logprob_bwd_kernel, the
// same bits for the same operands.  The conventions are grpo.hip's: fp32 arithmetic, 16-byte loads on rows of a 16-byte pitch, 64-bit row addresses,
// a fixed reduction order (per thread, per wave, the waves in order), no atomics.  The shift by one position is in the addressing: row (b, s) reads the
// label ids[b, s + 1]; rows s = S - 1 are not read by the forward and become exact zeros in the backward.
#include <math.h>

#include "rows_bf16.h"

namespace {

// (maximum, sum of exp(x - maximum)) of one chunk row by a 256-thread block: online over 16-byte pieces, a scalar tail for Vc % 8, then the waves in
// order.  -inf entries are legal; a thread, wave or row that saw none but -inf carries (-inf, 0).
__device__ __forceinline__ void chunk_max_sum_256(const bf16_t* __restrict__ lr, int64_t Vc, float* red_m, float* red_s, float& cm, float& cs) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float m = -INFINITY, s = 0.f;
    const int64_t nv = Vc >> 3;
    for (int64_t i = threadIdx.x; i < nv; i += 256) {
        float v[8];
        unpack8(*reinterpret_cast<const u32x4*>(lr + i * 8), v);
        float vm = v[0];
#pragma unroll
        for (int e = 1; e < 8; ++e) vm = fmaxf(vm, v[e]);
        if (vm > m) {
            s *= __expf(m - vm);
            m = vm;
        }
        if (m != -INFINITY) {
#pragma unroll
            for (int e = 0; e < 8; ++e) s += __expf(v[e] - m);
        }
    }
    for (int64_t i = (nv << 3) + threadIdx.x; i < Vc; i += 256) {
        const float v = bf2f(lr[i]);
        if (v > m) {
            s *= __expf(m - v);
            m = v;
        }
        if (m != -INFINITY) s += __expf(v - m);
    }
    const float wm = wave_max(m);
    s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
    __syncthreads();  // protects red_* reuse across rows
    if (lane == 0) {
        red_m[wid] = wm;
        red_s[wid] = s;
    }
    __syncthreads();
    cm = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    cs = 0.f;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) cs += red_m[wv] == -INFINITY ? 0.f : red_s[wv] * __expf(red_m[wv] - cm);
}

// One chunk's share of the running (m, l): l counts exp(x - m) over the columns seen so far.  A side whose maximum is still -inf holds nothing and is
// left out (exp(-inf - -inf) would be NaN): a row whose first chunks are all -inf gives the lse of its finite part.
__global__ __launch_bounds__(256) void head_lse_chunk_kernel(int64_t rows, int64_t S, int64_t Vc, int64_t c0, const bf16_t* __restrict__ chunk,
                                                             int64_t ldc, const int64_t* __restrict__ ids, float* __restrict__ m_state,
                                                             float* __restrict__ l_state, float* __restrict__ label_logit, int first) {
    __shared__ float red_m[4], red_s[4];
    const int64_t T = S - 1;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / T, s = row - b * T;
        const bf16_t* lr = chunk + (b * S + s) * ldc;
        float cm, cs;
        chunk_max_sum_256(lr, Vc, red_m, red_s, cm, cs);
        if (threadIdx.x == 0) {
            float m = cm, l = cs;
            if (!first) {
                const float mo = m_state[row], lo = l_state[row];
                m = fmaxf(mo, cm);
                l = (mo == -INFINITY ? 0.f : lo * expf(mo - m)) + (cm == -INFINITY ? 0.f : cs * expf(cm - m));
            }
            m_state[row] = m;
            l_state[row] = l;
            const int64_t tgt = ids[b * S + s + 1] - c0;
            if (tgt >= 0 && tgt < Vc) label_logit[row] = bf2f(lr[tgt]);
            else if (first) label_logit[row] = __builtin_nanf("");  // stays NaN when no chunk holds the label: a label outside [0, V)
        }
    }
}

__global__ __launch_bounds__(256) void head_lse_finish_kernel(int64_t n, const float* __restrict__ m_state, const float* __restrict__ l_state,
                                                              const float* __restrict__ label_logit, float* __restrict__ logp,
                                                              float* __restrict__ lse) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float z = m_state[i] + logf(l_state[i]);  // once per row: the accurate logarithm
        lse[i] = z;
        logp[i] = label_logit[i] - z;
    }
}

// dchunk[b, s, j] = bf16(g[b, s] (onehot(ids[b, s + 1] - c0)[j] - exp(chunk[b, s, j] - lse[b, s]))) for s < S - 1; rows S - 1, and the row of a label
// outside [0, V), are exact zeros.  src == dst is allowed (each element is read, then written, by one thread).  c0 is a multiple of 8, so a column is
// on the 16-byte path here exactly when it is in label_logprob_bwd_kernel over the whole row; both paths evaluate the one expression below.
__global__ __launch_bounds__(256) void head_dlogits_chunk_kernel(int64_t rows, int64_t S, int64_t V, int64_t Vc, int64_t c0, const float* __restrict__ g,
                                                                 const bf16_t* chunk, int64_t ldc, const float* __restrict__ lse,
                                                                 const int64_t* __restrict__ ids, bf16_t* dchunk, int64_t ldd) {
    const int64_t T = S - 1, nv = Vc >> 3;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int64_t b = row / S, s = row - b * S;
        const bf16_t* lr = chunk + row * ldc;
        bf16_t* dr = dchunk + row * ldd;
        const int64_t label = s < T ? ids[b * S + s + 1] : -1;
        if (label < 0 || label >= V) {
            for (int64_t i = threadIdx.x; i < nv; i += 256) *reinterpret_cast<u32x4*>(dr + i * 8) = (u32x4){0, 0, 0, 0};
            for (int64_t i = (nv << 3) + threadIdx.x; i < Vc; i += 256) dr[i] = 0;
            continue;
        }
        const int64_t tgt = label - c0;  // outside [0, Vc): no column of this chunk matches
        const float z = lse[b * T + s], w = g[b * T + s];
        for (int64_t i = threadIdx.x; i < nv; i += 256) {
            float v[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(lr + i * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = w * (((i * 8 + e) == tgt ? 1.0f : 0.0f) - __expf(v[e] - z));
            *reinterpret_cast<u32x4*>(dr + i * 8) = pack8(o);
        }
        for (int64_t i = (nv << 3) + threadIdx.x; i < Vc; i += 256) dr[i] = f2bf(w * ((i == tgt ? 1.0f : 0.0f) - __expf(bf2f(lr[i]) - z)));
    }
}

bool head_chunk_ok(const char* name, int64_t B, int64_t S, int64_t Vc, int64_t c0, const void* chunk, int64_t ldc) {
    if (!(B > 0 && B <= (1 << 24) && S >= 2 && S <= (1 << 24) && Vc > 0 && Vc <= (int64_t)1 << 31 && c0 >= 0 && c0 <= (int64_t)1 << 31 && chunk)) {
        mi355_set_error("%s: bad arguments (B in 1..2^24, S in 2..2^24, Vc in 1..2^31, c0 in 0..2^31, non-null pointers)", name);
        return false;
    }
    if (!(ldc >= Vc && (ldc & 7) == 0 && (c0 & 7) == 0 && ((uintptr_t)chunk & 15) == 0)) {
        mi355_set_error("%s: the vector path needs 16-byte rows: pointer 16-byte aligned, row pitch >= Vc and c0 multiples of 8 elements", name);
        return false;
    }
    if (!(ldc <= (int64_t)1 << 32 && B * S <= ((int64_t)1 << 61) / ldc)) {
        mi355_set_error("%s: B S rows of pitch %ld do not fit a 64-bit element offset", name, (long)ldc);
        return false;
    }
    return true;
}

}  // namespace

#define STREAM ((hipStream_t)stream)

extern "C" int mi355_head_lse_chunk(int64_t B, int64_t S, int64_t Vc, int64_t c0, const void* chunk, int64_t ldc, const int64_t* ids, float* m, float* l,
                                    float* label_logit, int first, void* stream) {
    if (!head_chunk_ok("mi355_head_lse_chunk", B, S, Vc, c0, chunk, ldc)) return 1;
    MI355_REQUIRE(ids && m && l && label_logit, "mi355_head_lse_chunk: bad arguments (null pointer)");
    const int64_t rows = B * (S - 1);
    hipLaunchKernelGGL(head_lse_chunk_kernel, dim3((unsigned)(rows < 65535 ? rows : 65535)), dim3(256), 0, STREAM, rows, S, Vc, c0, (const bf16_t*)chunk, ldc,
                       ids, m, l, label_logit, first != 0);
    MI355_LAUNCH_CHECK("mi355_head_lse_chunk");
    return 0;
}

extern "C" int mi355_head_lse_finish(int64_t n, const float* m, const float* l, const float* label_logit, float* logp, float* lse, void* stream) {
    MI355_REQUIRE(n > 0 && n <= (int64_t)1 << 48 && m && l && label_logit && logp && lse,
                  "mi355_head_lse_finish: bad arguments (n = B (S - 1) in 1..2^48, non-null pointers)");
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(head_lse_finish_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, STREAM, n, m, l, label_logit, logp, lse);
    MI355_LAUNCH_CHECK("mi355_head_lse_finish");
    return 0;
}

extern "C" int mi355_head_dlogits_chunk(int64_t B, int64_t S, int64_t V, int64_t Vc, int64_t c0, const float* g, const void* chunk, int64_t ldc,
                                        const float* lse, const int64_t* ids, void* dchunk, int64_t ldd, void* stream) {
    if (!head_chunk_ok("mi355_head_dlogits_chunk", B, S, Vc, c0, chunk, ldc)) return 1;
    if (!head_chunk_ok("mi355_head_dlogits_chunk", B, S, Vc, c0, dchunk, ldd)) return 1;
    MI355_REQUIRE(V > 0 && V <= (int64_t)1 << 31 && c0 + Vc <= V, "mi355_head_dlogits_chunk: the chunk [c0, c0 + Vc) must lie inside the vocabulary (V in 1..2^31)");
    MI355_REQUIRE(g && lse && ids, "mi355_head_dlogits_chunk: bad arguments (null pointer)");
    MI355_REQUIRE(dchunk != chunk || ldd == ldc, "mi355_head_dlogits_chunk: in place needs the chunk's own pitch");
    const int64_t rows = B * S;
    hipLaunchKernelGGL(head_dlogits_chunk_kernel, dim3((unsigned)(rows < 65535 ? rows : 65535)), dim3(256), 0, STREAM, rows, S, V, Vc, c0, g,
                       (const bf16_t*)chunk, ldc, lse, ids, (bf16_t*)dchunk, ldd);
    MI355_LAUNCH_CHECK("mi355_head_dlogits_chunk");
    return 0;
}
