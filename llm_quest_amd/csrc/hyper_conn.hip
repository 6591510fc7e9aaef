// Hyper-connections (classic "hc", reference common/hyper_connections/hyper_connections.py + hyper_qwen3.py:134-165): the row work on the
// n-times-wider residual stream X [T, n, d] around one sub-layer, fused so that the streams are read once and written once on each side of it.
//
// Work split of the two "width" kernels: a workgroup owns one token at a time and a THREAD owns one 16-byte column vector (8 bf16) of every stream
// of that token (blockDim = d / 8 rounded up to a wave, <= 512 threads, so d <= 4096; up to d = 2048 the kernels are compiled for 256 threads, which
// gives a thread the whole register file of its SIMD -- the 512-thread variants of the n = 4 kernels spill to scratch).  Everything indexed by the stream number lives in
// registers (n is a template parameter), the per-column weights are loaded once per workgroup and stay in registers while it walks its tokens,
// the full-row reductions (sums of squares, the (n + 2) * n dot products) are wave shuffles + one LDS exchange between the waves, summed in a
// fixed order.  The column-wise parameter gradients of the backward therefore never cross threads: a thread accumulates its own columns over the
// workgroup's tokens and writes them into the workgroup's row of partials; mi355_reduce_rows_f32 folds the rows.  No atomics anywhere.
#include "rows_bf16.h"

namespace {

constexpr int HC_MAX_THREADS = 512;
constexpr int HC_SMALL_THREADS = 256;  // d <= 2048

// element e (a compile-time constant after unrolling) of 8 packed bf16: the streams stay packed in registers and are widened where they are used
__device__ __forceinline__ float el(const u32x4 v, int e) { return __uint_as_float((e & 1) ? (v[e >> 1] & 0xffff0000u) : (v[e >> 1] << 16)); }
__device__ __forceinline__ void load8f(const float* p, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = a[e], f[4 + e] = b[e];
}
__device__ __forceinline__ void store8f(float* p, const float (&f)[8]) {
    *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

// v[m] <- sum over the whole workgroup, the same bits in every thread: wave shuffles, then the waves' sums through `lds` ([waves][M])
// added in wave order.  One barrier per call: successive calls must alternate between two LDS regions (a wave can reach the call after the
// next only once every wave has passed the next call's barrier, i.e. has finished reading this one's region).
template <int M>
__device__ __forceinline__ void block_sum(float (&v)[M], float* lds) {
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = wave_sum(v[m]);
    const int nw = blockDim.x >> 6;
    if (nw == 1) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) lds[wv * M + m] = v[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m) {
        float s = lds[m];
        for (int w = 1; w < nw; ++w) s += lds[w * M + m];
        v[m] = s;
    }
}

// ------------------------------------------------------------------------------------------- width connection, forward
// One read of X; writes R [T,N,d], P [T,d], the coefficients H [T,N+2,N] (rows 0..N-1 H_res, row N h_pre, row N+1 h_post), the tanh values of
// the same shape and rstd [T,N].
template <int N, int MAXT>
__global__ __launch_bounds__(MAXT) void hc_width_fwd_kernel(int64_t T, int d, const bf16_t* __restrict__ X, const bf16_t* __restrict__ w_norm,
                                                                      const float* __restrict__ W_res, const float* __restrict__ w_pre,
                                                                      const float* __restrict__ w_post, const float* __restrict__ f_res,
                                                                      const float* __restrict__ f_pre, const float* __restrict__ f_post,
                                                                      const float* __restrict__ b_res, const float* __restrict__ b_pre,
                                                                      const float* __restrict__ b_post, bf16_t* __restrict__ R, bf16_t* __restrict__ P,
                                                                      float* __restrict__ H, float* __restrict__ TH, float* __restrict__ rstd, float eps) {
    constexpr int C = N + 2;  // coefficient rows: N of H_res, h_pre, h_post
    __shared__ float red[2][MAXT / 64 * C * N];
    const int col = threadIdx.x * 8;
    const bool active = col < d;
    float wc[C][8], wn[8];  // rows 0..N-1 W_res, N w_pre, N+1 w_post; RMSNorm weight
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) wc[c][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) wn[e] = 0.f;
    if (active) {
#pragma unroll
        for (int i = 0; i < N; ++i) load8f(W_res + (int64_t)i * d + col, wc[i]);
        load8f(w_pre + col, wc[N]);
        load8f(w_post + col, wc[N + 1]);
        unpack8(*reinterpret_cast<const u32x4*>(w_norm + col), wn);
    }
    const float fac[3] = {f_res[0], f_pre[0], f_post[0]};

    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        u32x4 x[N];
        float ss[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            x[j] = u32x4{0u, 0u, 0u, 0u};
            if (active) x[j] = *reinterpret_cast<const u32x4*>(X + (t * N + j) * d + col);
            ss[j] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) ss[j] += el(x[j], e) * el(x[j], e);
        }
        block_sum<N>(ss, red[0]);
        float r[N], z[C * N];  // z[c * N + j] = <xn[j], W_c>
#pragma unroll
        for (int k = 0; k < C * N; ++k) z[k] = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            r[j] = rsqrtf(ss[j] / (float)d + eps);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xn = rbf(el(x[j], e) * r[j] * wn[e]);  // the reference's bf16 norm output, cast back up for the dot products
#pragma unroll
                for (int c = 0; c < C; ++c) z[c * N + j] += xn * wc[c][e];
            }
        }
        block_sum<C * N>(z, red[1]);
        float h[C * N];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float f = fac[c < N ? 0 : c - N + 1];
            const float* b = c < N ? (b_res ? b_res + c * N : nullptr) : (c == N ? b_pre : b_post);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z[c * N + j] = tanhf(z[c * N + j]);
                h[c * N + j] = z[c * N + j] * f;
                if (b) h[c * N + j] += b[j];
            }
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < C * N; ++k) {
                H[t * (C * N) + k] = h[k];
                TH[t * (C * N) + k] = z[k];
            }
#pragma unroll
            for (int j = 0; j < N; ++j) rstd[t * N + j] = r[j];
        }
        if (active) {
            float o[8];
#pragma unroll
            for (int i = 0; i < N; ++i) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float s = h[i * N] * el(x[0], e);
#pragma unroll
                    for (int j = 1; j < N; ++j) s += h[i * N + j] * el(x[j], e);
                    o[e] = s;
                }
                *reinterpret_cast<u32x4*>(R + (t * N + i) * d + col) = pack8(o);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float s = h[N * N] * el(x[0], e);
#pragma unroll
                for (int j = 1; j < N; ++j) s += h[N * N + j] * el(x[j], e);
                o[e] = s;
            }
            *reinterpret_cast<u32x4*>(P + t * d + col) = pack8(o);
        }
    }
}

// ------------------------------------------------------------------------------------------- width connection, backward
// Row of partials of one workgroup (fp32, width hc_partial_width(N, d)):
//   [dW_res N*d | dw_pre d | dw_post d | dw_norm d | dfactor_res, dfactor_pre, dfactor_post | db_res N*N | db_pre N | db_post N | zero padding to 8]
__host__ __device__ constexpr int hc_tail(int n) { return (3 + n * n + 2 * n + 7) / 8 * 8; }
__host__ __device__ constexpr int64_t hc_partial_width(int n, int d) { return (int64_t)(n + 3) * d + hc_tail(n); }

template <int N, int MAXT>
__global__ __launch_bounds__(MAXT) void hc_width_bwd_kernel(int64_t T, int d, const bf16_t* __restrict__ dR, const bf16_t* __restrict__ dP,
                                                                      const float* __restrict__ dh_post, const bf16_t* __restrict__ X,
                                                                      const float* __restrict__ H, const float* __restrict__ TH,
                                                                      const float* __restrict__ rstd, const bf16_t* __restrict__ w_norm,
                                                                      const float* __restrict__ W_res, const float* __restrict__ w_pre,
                                                                      const float* __restrict__ w_post, const float* __restrict__ f_res,
                                                                      const float* __restrict__ f_pre, const float* __restrict__ f_post,
                                                                      bf16_t* __restrict__ dX, float* __restrict__ partial) {
    constexpr int C = N + 2;
    constexpr int NRED = N * N + N + C * N;  // dH_res, dh_pre, q
    __shared__ float red[2][MAXT / 64 * NRED];
    const int col = threadIdx.x * 8;
    const bool active = col < d;
    float wc[C][8], wn[8], aw[C][8], awn[8];  // weights of this thread's columns; their gradient accumulators
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) wc[c][e] = 0.f, aw[c][e] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) wn[e] = 0.f, awn[e] = 0.f;
    if (active) {
#pragma unroll
        for (int i = 0; i < N; ++i) load8f(W_res + (int64_t)i * d + col, wc[i]);
        load8f(w_pre + col, wc[N]);
        load8f(w_post + col, wc[N + 1]);
        unpack8(*reinterpret_cast<const u32x4*>(w_norm + col), wn);
    }
    const float fac[3] = {f_res[0], f_pre[0], f_post[0]};
    float ascal = 0.f;  // scalar gradients: thread k < C*N owns db[k], threads C*N .. C*N+2 the three dfactor (every thread sees the same dH)

    int flip = 0;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x, flip ^= 1) {
        u32x4 x[N], g[N], gp = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < N; ++j) {
            x[j] = g[j] = u32x4{0u, 0u, 0u, 0u};
            if (active) {
                x[j] = *reinterpret_cast<const u32x4*>(X + (t * N + j) * d + col);
                g[j] = *reinterpret_cast<const u32x4*>(dR + (t * N + j) * d + col);
            }
        }
        if (active) gp = *reinterpret_cast<const u32x4*>(dP + t * d + col);
        float h[C * N], th[C * N], r[N];
#pragma unroll
        for (int k = 0; k < C * N; ++k) h[k] = H[t * (C * N) + k], th[k] = TH[t * (C * N) + k];
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = rstd[t * N + j];

        // full-row sums: dH_res[i][j] = <dR[i], X[j]>, dh_pre[j] = <dP, X[j]>, q[c][j] = <W_c * w_norm, X[j]> (the RMSNorm backward's row
        // mean is sum_c dz[c][j] * q[c][j]: taking it from q keeps the kernel at ONE exchange between the waves per token)
        float s[NRED];
#pragma unroll
        for (int k = 0; k < NRED; ++k) s[k] = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float xe = el(x[j], e), xw = xe * wn[e];  // (x * w_norm) * W_c: no token-independent product for the compiler to keep in registers
#pragma unroll
                for (int i = 0; i < N; ++i) s[i * N + j] += el(g[i], e) * xe;
                s[N * N + j] += el(gp, e) * xe;
#pragma unroll
                for (int c = 0; c < C; ++c) s[N * N + N + c * N + j] += xw * wc[c][e];
            }
        }
        block_sum<NRED>(s, red[flip]);

        float dz[C * N], dot[N], dfac[3] = {0.f, 0.f, 0.f}, mine = 0.f;
#pragma unroll
        for (int j = 0; j < N; ++j) dot[j] = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int k = c * N + j;
                const float dh = c <= N ? s[k] : dh_post[t * N + j];  // rows 0..N of s are dH_res and dh_pre, in H's order
                dfac[c < N ? 0 : c - N + 1] += dh * th[k];
                mine = (int)threadIdx.x == k ? dh : mine;
                dz[k] = dh * fac[c < N ? 0 : c - N + 1] * (1.0f - th[k] * th[k]);
                dot[j] += dz[k] * s[N * N + N + k];
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) mine = (int)threadIdx.x == C * N + q ? dfac[q] : mine;
        ascal += mine;
#pragma unroll
        for (int j = 0; j < N; ++j) dot[j] = dot[j] * r[j] * r[j] / (float)d;

        if (active) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float xe = el(x[j], e), xr = xe * r[j];
                    const float xn = rbf(xr * wn[e]);
                    float dxn = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        dxn += dz[c * N + j] * wc[c][e];
                        aw[c][e] += dz[c * N + j] * xn;
                    }
                    awn[e] += dxn * xr;
                    float acc = h[j] * el(g[0], e);  // H_res[i][j] multiplies stream j into output stream i: its transpose carries dR back
#pragma unroll
                    for (int i = 1; i < N; ++i) acc += h[i * N + j] * el(g[i], e);
                    acc += h[N * N + j] * el(gp, e);
                    o[e] = acc + r[j] * (dxn * wn[e] - xe * dot[j]);
                }
                *reinterpret_cast<u32x4*>(dX + (t * N + j) * d + col) = pack8(o);
            }
        }
    }

    float* row = partial + (int64_t)blockIdx.x * hc_partial_width(N, d);
    if (active) {
#pragma unroll
        for (int c = 0; c < C; ++c) store8f(row + (int64_t)c * d + col, aw[c]);
        store8f(row + (int64_t)C * d + col, awn);
    }
    // blockDim >= 64 > hc_tail(N): the first threads write the scalar tail, [dfactor x3 | db C*N | zeros]
    if ((int)threadIdx.x < hc_tail(N)) {
        const int k = (int)threadIdx.x;
        float* tail = row + (int64_t)(C + 1) * d;
        const int dst = k < C * N ? 3 + k : (k < C * N + 3 ? k - C * N : k);
        tail[dst] = k < C * N + 3 ? ascal : 0.f;
    }
}

// ------------------------------------------------------------------------------------------- depth connection
// Out[t,i,:] = bf16( fp32(bf16(h_post[t,i] * Y[t,:])) + fp32(R[t,i,:]) ): one thread per (token, column vector).  Out may be R itself (a thread
// reads the vectors it writes before writing them), so neither is __restrict__.
template <int N>
__global__ __launch_bounds__(256) void hc_depth_fwd_kernel(int64_t T, int d, const bf16_t* __restrict__ Y, const float* __restrict__ h_post, int64_t ldh,
                                                           const bf16_t* R, bf16_t* Out) {
    const int nvec = d >> 3;
    const int64_t total = T * nvec;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t t = idx / nvec;
        const int col = (int)(idx - t * nvec) * 8;
        float y[8];
        unpack8(*reinterpret_cast<const u32x4*>(Y + t * d + col), y);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float hp = h_post[t * ldh + i];
            float rv[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(R + (t * N + i) * d + col), rv);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = rbf(hp * y[e]) + rv[e];
            *reinterpret_cast<u32x4*>(Out + (t * N + i) * d + col) = pack8(o);
        }
    }
}

// dY[t,:] = bf16(sum_i h_post[t,i] * dOut[t,i,:]), dh_post[t,i] = <dOut[t,i,:], Y[t,:]>: one wave per token, four tokens per workgroup.
template <int N>
__global__ __launch_bounds__(256) void hc_depth_bwd_kernel(int64_t T, int d, const bf16_t* __restrict__ dOut, const bf16_t* __restrict__ Y,
                                                           const float* __restrict__ h_post, int64_t ldh, bf16_t* __restrict__ dY,
                                                           float* __restrict__ dh_post) {
    const int lane = threadIdx.x & 63;
    const int nvec = d >> 3;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += (int64_t)gridDim.x * 4) {
        float hp[N], dh[N];
#pragma unroll
        for (int i = 0; i < N; ++i) hp[i] = h_post[t * ldh + i], dh[i] = 0.f;
        for (int v = lane; v < nvec; v += 64) {
            float y[8], o[8];
            unpack8(*reinterpret_cast<const u32x4*>(Y + t * d + v * 8), y);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                float gi[8];
                unpack8(*reinterpret_cast<const u32x4*>(dOut + (t * N + i) * d + v * 8), gi);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    o[e] += hp[i] * gi[e];
                    dh[i] += gi[e] * y[e];
                }
            }
            *reinterpret_cast<u32x4*>(dY + t * d + v * 8) = pack8(o);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) dh[i] = wave_sum(dh[i]);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < N; ++i) dh_post[t * N + i] = dh[i];
        }
    }
}

// ------------------------------------------------------------------------------------------- entering and leaving the streams
// SUM: out[t,:] = bf16(sum_j X[t,j,:]) (fp32 accumulation in stream order, one rounding); otherwise out[t,j,:] = x[t,:] for every j.
template <int N, bool SUM>
__global__ __launch_bounds__(256) void hc_stream_kernel(int64_t T, int d, const bf16_t* __restrict__ in, bf16_t* __restrict__ out) {
    const int nvec = d >> 3;
    const int64_t total = T * nvec;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t t = idx / nvec;
        const int col = (int)(idx - t * nvec) * 8;
        if (SUM) {
            float acc[8], v[8];
            unpack8(*reinterpret_cast<const u32x4*>(in + (t * N) * d + col), acc);
#pragma unroll
            for (int j = 1; j < N; ++j) {
                unpack8(*reinterpret_cast<const u32x4*>(in + (t * N + j) * d + col), v);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += v[e];
            }
            *reinterpret_cast<u32x4*>(out + t * d + col) = pack8(acc);
        } else {
            const u32x4 v = *reinterpret_cast<const u32x4*>(in + t * d + col);
#pragma unroll
            for (int j = 0; j < N; ++j) *reinterpret_cast<u32x4*>(out + (t * N + j) * d + col) = v;
        }
    }
}

// Shape rules shared by every entry point.  Returns 0 when the launch may go ahead, 1 on a refusal (message set), -1 for an empty problem.
int hc_check(const char* name, int64_t T, int n, int d, int d_max) {
    if (n != 2 && n != 4) {
        mi355_set_error("%s: expansion rate n must be 2 or 4 (got %d)", name, n);
        return 1;
    }
    if (d <= 0 || (d & 7) != 0 || d > d_max) {
        mi355_set_error("%s: emb_dim d must be a positive multiple of 8, at most %d (got %d)", name, d_max, d);
        return 1;
    }
    if (T > ((int64_t)1 << 40)) {
        mi355_set_error("%s: token count %lld out of range", name, (long long)T);
        return 1;
    }
    return T <= 0 ? -1 : 0;
}
constexpr int HC_WIDTH_D_MAX = HC_MAX_THREADS * 8;  // a thread per 16-byte column vector
constexpr int HC_FLAT_D_MAX = 1 << 20;
inline unsigned hc_width_threads(int d) { return (unsigned)(((d >> 3) + 63) / 64 * 64); }
inline unsigned hc_flat_grid(int64_t T, int d) {
    const int64_t blocks = (T * (d >> 3) + 255) / 256;
    return (unsigned)(blocks < 8192 ? blocks : 8192);
}

}  // namespace

#define HC_DISPATCH(n, call2, call4) \
    do {                             \
        if ((n) == 2) {              \
            call2;                   \
        } else {                     \
            call4;                   \
        }                            \
    } while (0)

extern "C" int mi355_hc_width_fwd(int64_t T, int n, int d, const void* X, const void* w_norm, const float* W_res, const float* w_pre, const float* w_post,
                                  const float* factor_res, const float* factor_pre, const float* factor_post, const float* bias_res,
                                  const float* bias_pre, const float* bias_post, void* R, void* P, float* H, float* TH, float* rstd, float eps,
                                  int max_blocks, void* stream) {
    const int rc = hc_check("mi355_hc_width_fwd", T, n, d, HC_WIDTH_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(X && w_norm && W_res && w_pre && w_post && factor_res && factor_pre && factor_post && R && P && H && TH && rstd,
                  "mi355_hc_width_fwd: null pointer (only the three biases may be null)");
    MI355_REQUIRE(max_blocks > 0, "mi355_hc_width_fwd: max_blocks must be positive (got %d)", max_blocks);
    const unsigned grid = (unsigned)(T < max_blocks ? T : max_blocks), threads = hc_width_threads(d);
    hipStream_t s = (hipStream_t)stream;
#define HC_WF(NN, MT)                                                                                                                            \
    hipLaunchKernelGGL((hc_width_fwd_kernel<NN, MT>), dim3(grid), dim3(threads), 0, s, T, d, (const bf16_t*)X, (const bf16_t*)w_norm, W_res, w_pre, \
                       w_post, factor_res, factor_pre, factor_post, bias_res, bias_pre, bias_post, (bf16_t*)R, (bf16_t*)P, H, TH, rstd, eps)
    if (threads <= HC_SMALL_THREADS)
        HC_DISPATCH(n, HC_WF(2, HC_SMALL_THREADS), HC_WF(4, HC_SMALL_THREADS));
    else
        HC_DISPATCH(n, HC_WF(2, HC_MAX_THREADS), HC_WF(4, HC_MAX_THREADS));
#undef HC_WF
    MI355_LAUNCH_CHECK("mi355_hc_width_fwd");
    return 0;
}

extern "C" int64_t mi355_hc_width_bwd_partial_width(int n, int d) {
    if ((n != 2 && n != 4) || d <= 0 || (d & 7) != 0 || d > HC_WIDTH_D_MAX) return 0;
    return hc_partial_width(n, d);
}

extern "C" int mi355_hc_width_bwd(int64_t T, int n, int d, const void* dR, const void* dP, const float* dh_post, const void* X, const float* H,
                                  const float* TH, const float* rstd, const void* w_norm, const float* W_res, const float* w_pre, const float* w_post,
                                  const float* factor_res, const float* factor_pre, const float* factor_post, void* dX, float* partial, int parts,
                                  void* stream) {
    const int rc = hc_check("mi355_hc_width_bwd", T, n, d, HC_WIDTH_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(dR && dP && dh_post && X && H && TH && rstd && w_norm && W_res && w_pre && w_post && factor_res && factor_pre && factor_post && dX &&
                      partial,
                  "mi355_hc_width_bwd: null pointer");
    MI355_REQUIRE(parts > 0 && parts <= T, "mi355_hc_width_bwd: parts must be in [1, T] (every row of partials is written by a workgroup that owns a token; got %d for %lld tokens)",
                  parts, (long long)T);
    const unsigned threads = hc_width_threads(d);
    hipStream_t s = (hipStream_t)stream;
#define HC_WB(NN, MT)                                                                                                                             \
    hipLaunchKernelGGL((hc_width_bwd_kernel<NN, MT>), dim3((unsigned)parts), dim3(threads), 0, s, T, d, (const bf16_t*)dR, (const bf16_t*)dP,        \
                       dh_post, (const bf16_t*)X, H, TH, rstd, (const bf16_t*)w_norm, W_res, w_pre, w_post, factor_res, factor_pre, factor_post, \
                       (bf16_t*)dX, partial)
    if (threads <= HC_SMALL_THREADS)
        HC_DISPATCH(n, HC_WB(2, HC_SMALL_THREADS), HC_WB(4, HC_SMALL_THREADS));
    else
        HC_DISPATCH(n, HC_WB(2, HC_MAX_THREADS), HC_WB(4, HC_MAX_THREADS));
#undef HC_WB
    MI355_LAUNCH_CHECK("mi355_hc_width_bwd");
    return 0;
}

extern "C" int mi355_hc_depth_fwd(int64_t T, int n, int d, const void* Y, const float* h_post, int64_t ldh, const void* R, void* Out, void* stream) {
    const int rc = hc_check("mi355_hc_depth_fwd", T, n, d, HC_FLAT_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(Y && h_post && R && Out, "mi355_hc_depth_fwd: null pointer");
    MI355_REQUIRE(ldh >= n, "mi355_hc_depth_fwd: h_post token stride %lld is smaller than n = %d", (long long)ldh, n);
    const unsigned grid = hc_flat_grid(T, d);
    hipStream_t s = (hipStream_t)stream;
    HC_DISPATCH(n, hipLaunchKernelGGL(hc_depth_fwd_kernel<2>, dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)Y, h_post, ldh, (const bf16_t*)R, (bf16_t*)Out),
                hipLaunchKernelGGL(hc_depth_fwd_kernel<4>, dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)Y, h_post, ldh, (const bf16_t*)R, (bf16_t*)Out));
    MI355_LAUNCH_CHECK("mi355_hc_depth_fwd");
    return 0;
}

extern "C" int mi355_hc_depth_bwd(int64_t T, int n, int d, const void* dOut, const void* Y, const float* h_post, int64_t ldh, void* dY, float* dh_post,
                                  void* stream) {
    const int rc = hc_check("mi355_hc_depth_bwd", T, n, d, HC_FLAT_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(dOut && Y && h_post && dY && dh_post, "mi355_hc_depth_bwd: null pointer");
    MI355_REQUIRE(ldh >= n, "mi355_hc_depth_bwd: h_post token stride %lld is smaller than n = %d", (long long)ldh, n);
    const int64_t blocks = (T + 3) / 4;
    const unsigned grid = (unsigned)(blocks < 4096 ? blocks : 4096);
    hipStream_t s = (hipStream_t)stream;
    HC_DISPATCH(n, hipLaunchKernelGGL(hc_depth_bwd_kernel<2>, dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)dOut, (const bf16_t*)Y, h_post, ldh, (bf16_t*)dY, dh_post),
                hipLaunchKernelGGL(hc_depth_bwd_kernel<4>, dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)dOut, (const bf16_t*)Y, h_post, ldh, (bf16_t*)dY, dh_post));
    MI355_LAUNCH_CHECK("mi355_hc_depth_bwd");
    return 0;
}

extern "C" int mi355_hc_stream_sum(int64_t T, int n, int d, const void* X, void* out, void* stream) {
    const int rc = hc_check("mi355_hc_stream_sum", T, n, d, HC_FLAT_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(X && out, "mi355_hc_stream_sum: null pointer");
    const unsigned grid = hc_flat_grid(T, d);
    hipStream_t s = (hipStream_t)stream;
    HC_DISPATCH(n, hipLaunchKernelGGL((hc_stream_kernel<2, true>), dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)X, (bf16_t*)out),
                hipLaunchKernelGGL((hc_stream_kernel<4, true>), dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)X, (bf16_t*)out));
    MI355_LAUNCH_CHECK("mi355_hc_stream_sum");
    return 0;
}

extern "C" int mi355_hc_stream_broadcast(int64_t T, int n, int d, const void* x, void* out, void* stream) {
    const int rc = hc_check("mi355_hc_stream_broadcast", T, n, d, HC_FLAT_D_MAX);
    if (rc) return rc < 0 ? 0 : rc;
    MI355_REQUIRE(x && out, "mi355_hc_stream_broadcast: null pointer");
    const unsigned grid = hc_flat_grid(T, d);
    hipStream_t s = (hipStream_t)stream;
    HC_DISPATCH(n, hipLaunchKernelGGL((hc_stream_kernel<2, false>), dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)x, (bf16_t*)out),
                hipLaunchKernelGGL((hc_stream_kernel<4, false>), dim3(grid), dim3(256), 0, s, T, d, (const bf16_t*)x, (bf16_t*)out));
    MI355_LAUNCH_CHECK("mi355_hc_stream_broadcast");
    return 0;
}
