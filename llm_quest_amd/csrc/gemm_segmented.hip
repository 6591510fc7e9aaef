// Segmented GEMM for the mixture-of-experts layers: mi355_gemm_bf16_segmented (row-segmented NT / NN) and mi355_gemm_bf16_segmented_tn (K-segmented TN).
//
// This translation unit is gemm.hip's eighth part: it includes gemm.hip with GEMM_PART = 7, which compiles none of that file's kernels or entry points
// (every instantiation there sits behind its own part number) and leaves its templates -- TileCfg, GemmParams, gemm_tile -- to the kernels below, which sit
// beside gemm_grouped_kernel in the same unnamed namespace.  They live in a file of their own so that the objects of gemm.hip, and the fingerprint of the
// headline step's kernel sources (llm_quest_amd/fingerprint.py), do not change with them.
#define GEMM_PART 7
#include "gemm.hip"

namespace {

// All experts of a MoE layer in ONE launch, the segment table read ON THE DEVICE: a workgroup builds its GemmParams from counts / offsets (what
// mi355_moe_plan left in device memory) and runs gemm_tile on them, so the sums, their K order and the epilogues are those of one mi355_gemm_bf16 call
// per expert on the 128x128 tile -- bit for bit -- and the host never learns the counts.  No atomics, no split-K, no workgroup waits for another.
constexpr int MAX_SEG = 128;
struct SegParams {
    GemmParams p;  // the operand bases, pitches and epilogue; row form: N, K (M comes from the counts), TN form: M, N (K comes from the counts)
    const int* counts;   // [E]
    const int* offsets;  // [>= E]: first row of each segment
    int E;
    int64_t rows;    // rows the caller declared for the row operands: a segment is clamped to them whatever the table holds
    int64_t stride;  // elements between two experts' B (row form) or C / residual (TN form)
};

// segment e as the kernels use it: inside [0, rows), never negative.  A row start keeps the 16-byte alignment of the DMA by the pitches alone (multiples of 8 elements).
__device__ __forceinline__ void seg_bounds(const SegParams& sp, int e, int& start, int& n) {
    const int64_t s = sp.offsets[e], c = sp.counts[e];
    const bool ok = s >= 0 && s < sp.rows && c > 0;
    start = ok ? (int)s : 0;
    n = ok ? (int)min(c, sp.rows - s) : 0;
}

// Row-segmented product (NT / NN): segment e = rows offsets[e] .. + counts[e] of A, C and the residual-slot operand, B_e = B + e * stride.  The grid is the static bound
// (max_rows / BM + min(E, max_rows)) * tiles_n >= sum_e ceil(counts[e] / BM) * tiles_n; every wave finds the expert of its row tile by a prefix sum of the
// experts' tile counts over its 64 lanes (two experts per lane), a workgroup beyond the last tile leaves at once.  A tile never crosses a segment.
template <class T, bool B_TR>
__global__ __launch_bounds__(T::NTHREADS, T::MIN_WAVES) void gemm_segmented_kernel(SegParams sp) {
    __shared__ __attribute__((aligned(16))) char smem[T::SMEM];
    static_assert(MAX_SEG == 128, "two experts per lane");
    const int lane = threadIdx.x & 63;
    const int tiles_n = sp.p.tiles_n;
    const int rt = blockIdx.x / tiles_n, tn = blockIdx.x - rt * tiles_n;
    int st[2], cn[2], incl[2], base = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int e = lane + 64 * h;
        st[h] = cn[h] = 0;
        if (e < sp.E) seg_bounds(sp, e, st[h], cn[h]);
        int s = (cn[h] + T::BM - 1) / T::BM;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(s, d, 64);
            if (lane >= d) s += o;
        }
        incl[h] = base + s;
        base += __shfl(s, 63, 64);
    }
    // the inclusive sums do not decrease: the experts whose sum is <= rt are exactly those in front of the one that owns row tile rt (empty ones skipped)
    int e = __popcll(__ballot(incl[0] <= rt));
    if (e == 64) e += __popcll(__ballot(incl[1] <= rt));
    if (e >= sp.E) return;
    const int hi = e >> 6, src = e & 63;
    const int start = __builtin_amdgcn_readfirstlane(__shfl(hi ? st[1] : st[0], src, 64));
    const int n = __builtin_amdgcn_readfirstlane(__shfl(hi ? cn[1] : cn[0], src, 64));
    const int last = __builtin_amdgcn_readfirstlane(__shfl(hi ? incl[1] : incl[0], src, 64));
    GemmParams p = sp.p;
    p.M = n;
    p.tiles_m = (n + T::BM - 1) / T::BM;
    const int tm = rt - (last - p.tiles_m);  // row tile inside the segment
    p.A += (int64_t)start * p.lda;
    p.B += (int64_t)e * sp.stride;
    p.C = reinterpret_cast<bf16_t*>(p.C) + (int64_t)start * p.ldc;
    if (p.R) p.R = reinterpret_cast<const bf16_t*>(p.R) + (int64_t)start * p.ldr;
    gemm_tile<T, false, B_TR, MI355_DT_BF16>(p, tm * tiles_n + tn, 0, smem);
}

// K-segmented product (TN, the experts' weight gradients): C_e = A_seg^T B_seg (+ residual_e) with K_e = counts[e]; the grid is E * tiles(M, N).  An expert without
// a row runs no K-tile: its accumulators stay zero and the write-out leaves exactly residual_e, or exactly zero.
template <class T, int OUT_DT>
__global__ __launch_bounds__(T::NTHREADS, T::MIN_WAVES) void gemm_segmented_tn_kernel(SegParams sp) {
    __shared__ __attribute__((aligned(16))) char smem[T::SMEM];
    const int per = sp.p.tiles_m * sp.p.tiles_n;
    const int e = blockIdx.x / per;
    if (e >= sp.E) return;
    int start, n;
    seg_bounds(sp, e, start, n);
    constexpr int64_t ES = OUT_DT == MI355_DT_BF16 ? 2 : 4;
    GemmParams p = sp.p;
    p.K = n;
    p.A += (int64_t)start * p.lda;
    p.B += (int64_t)start * p.ldb;
    p.C = reinterpret_cast<char*>(p.C) + (int64_t)e * sp.stride * ES;
    if (p.R) p.R = reinterpret_cast<const char*>(p.R) + (int64_t)e * sp.stride * ES;
    gemm_tile<T, true, true, OUT_DT>(p, blockIdx.x - e * per, 0, smem);
}

template <class T>
int launch_segmented(int form, SegParams& sp, int64_t max_rows, hipStream_t s) {
    sp.p.tiles_n = (int)((sp.p.N + T::BN - 1) / T::BN);
    // sum_e ceil(counts[e] / BM) <= max_rows / BM + (experts that hold a row), for every routing of max_rows assignments
    const int64_t row_tiles = max_rows / T::BM + (sp.E < max_rows ? sp.E : max_rows);
    const int64_t grid = row_tiles * sp.p.tiles_n;
    MI355_REQUIRE(grid < 0x7fffffffLL / 16, "mi355_gemm_bf16_segmented: grid too large");
    if (form == MI355_GEMM_NT)
        hipLaunchKernelGGL((gemm_segmented_kernel<T, false>), dim3((unsigned)grid), dim3(T::NTHREADS), 0, s, sp);
    else
        hipLaunchKernelGGL((gemm_segmented_kernel<T, true>), dim3((unsigned)grid), dim3(T::NTHREADS), 0, s, sp);
    MI355_LAUNCH_CHECK("mi355_gemm_bf16_segmented");
    return 0;
}

template <class T>
int launch_segmented_tn(SegParams& sp, int out_dtype, hipStream_t s) {
    sp.p.tiles_m = (int)((sp.p.M + T::BM - 1) / T::BM);
    sp.p.tiles_n = (int)((sp.p.N + T::BN - 1) / T::BN);
    const int64_t grid = (int64_t)sp.E * sp.p.tiles_m * sp.p.tiles_n;
    MI355_REQUIRE(grid < 0x7fffffffLL / 16, "mi355_gemm_bf16_segmented_tn: grid too large");
    if (out_dtype == MI355_DT_BF16)
        hipLaunchKernelGGL((gemm_segmented_tn_kernel<T, MI355_DT_BF16>), dim3((unsigned)grid), dim3(T::NTHREADS), 0, s, sp);
    else
        hipLaunchKernelGGL((gemm_segmented_tn_kernel<T, MI355_DT_F32>), dim3((unsigned)grid), dim3(T::NTHREADS), 0, s, sp);
    MI355_LAUNCH_CHECK("mi355_gemm_bf16_segmented_tn");
    return 0;
}

}  // namespace

static void seg_params_init(SegParams& sp, int E, const int32_t* counts, const int32_t* offsets, int64_t rows, int64_t stride) {
    GemmParams& p = sp.p;
    p.bias = nullptr; p.M = p.N = p.K = 0; p.tiles_m = p.tiles_n = 0; p.ksplit = 1; p.ws = nullptr; p.ablate = 0;
    p.ad_lse = nullptr; p.ad_delta = p.ad_nl2 = p.ad_ndl = nullptr; p.ad_S = p.ad_Hq = 0;
    p.split3 = 0;
    sp.counts = counts; sp.offsets = offsets; sp.E = E; sp.rows = rows; sp.stride = stride;
}

extern "C" int mi355_gemm_bf16_segmented(int form, int E, const int32_t* counts, const int32_t* offsets, int64_t max_rows, int64_t R, int64_t N, int64_t K,
                                         const void* A, int64_t lda, const void* B, int64_t ldb, int64_t strideB, void* C, int64_t ldc, void* residual,
                                         int64_t ldr, int epilogue, int tile_hint, void* stream) {
    const char* who = "mi355_gemm_bf16_segmented";
    MI355_REQUIRE(form == MI355_GEMM_NT || form == MI355_GEMM_NN, "%s: form must be NT or NN (got %d; the TN form is mi355_gemm_bf16_segmented_tn)", who, form);
    MI355_REQUIRE(E >= 1 && E <= MAX_SEG, "%s: E must be 1..%d, got %d", who, MAX_SEG, E);
    if (max_rows <= 0 || R <= 0) return 0;  // no assignment: nothing to write
    MI355_REQUIRE(N > 0 && K > 0, "%s: empty problem N=%ld K=%ld", who, (long)N, (long)K);
    MI355_REQUIRE(counts && offsets && A && B && C, "%s: null operand", who);
    MI355_REQUIRE((lda & 7) == 0 && (ldb & 7) == 0 && (ldc & 7) == 0 && (strideB & 7) == 0, "%s: lda / ldb / ldc / strideB must be multiples of 8 (16-byte rows)", who);
    MI355_REQUIRE((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0, "%s: A / B / C must be 16-byte aligned", who);
    MI355_REQUIRE((K & 7) == 0 && (N & 7) == 0, "%s: N, K must be multiples of 8", who);
    MI355_REQUIRE(lda >= K && ldb >= (form == MI355_GEMM_NT ? K : N) && strideB >= 0, "%s: a pitch is shorter than its row", who);
    MI355_REQUIRE(lda * 2 * 256 < 0x7fffffffLL && ldb * 2 * 256 < 0x7fffffffLL, "%s: leading dimension too large", who);
    MI355_REQUIRE(max_rows <= R && R < 0x7fffffffLL, "%s: max_rows = %ld assignments do not fit the R = %ld declared rows", who, (long)max_rows, (long)R);
    MI355_REQUIRE(tile_hint == 0 || tile_hint == 1, "%s: tile_hint must be 0 (auto) or 1 (128x128)", who);
    MI355_REQUIRE(epilogue == MI355_EPI_NONE || epilogue == MI355_EPI_SWIGLU_FWD || epilogue == MI355_EPI_SWIGLU_BWD, "%s: epilogue must be NONE, SWIGLU_FWD or SWIGLU_BWD, got %d", who, epilogue);
    if (residual) MI355_REQUIRE((ldr & 7) == 0 && ((uintptr_t)residual & 15) == 0, "%s: the residual-slot operand needs 16-byte aligned rows", who);
    if (epilogue == MI355_EPI_NONE) MI355_REQUIRE(ldc >= N && (!residual || ldr >= N), "%s: C / residual rows hold N columns", who);
    if (epilogue == MI355_EPI_SWIGLU_FWD)
        MI355_REQUIRE(form == MI355_GEMM_NT && residual && (N & 63) == 0 && ldc >= N && ldr >= N / 2,
                      "%s(SwiGLU forward epilogue): NT form, gate-up output [R, N] with N = 2F, F %% 32 == 0, `residual` = the activation output [R, F]", who);
    if (epilogue == MI355_EPI_SWIGLU_BWD)
        MI355_REQUIRE(form == MI355_GEMM_NN && residual && ldc >= 2 * N && ldr >= 2 * N,
                      "%s(SwiGLU backward epilogue): NN form, output [R, 2N] (ldc >= 2N), `residual` = the forward gate-up output [R, 2N]", who);
    SegParams sp;
    seg_params_init(sp, E, counts, offsets, R, strideB);
    GemmParams& p = sp.p;
    p.A = (const bf16_t*)A; p.B = (const bf16_t*)B; p.C = C; p.R = residual;
    p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldr = residual ? ldr : 0;
    p.epilogue = epilogue;
    return launch_segmented<Cfg128>(form, sp, max_rows, (hipStream_t)stream);
}

extern "C" int mi355_gemm_bf16_segmented_tn(int E, const int32_t* counts, const int32_t* offsets, int64_t R, int64_t M, int64_t N, const void* A, int64_t lda,
                                            const void* B, int64_t ldb, void* C, int64_t ldc, int64_t strideC, int out_dtype, const void* residual, int64_t ldr,
                                            int tile_hint, void* stream) {
    const char* who = "mi355_gemm_bf16_segmented_tn";
    MI355_REQUIRE(E >= 1 && E <= MAX_SEG, "%s: E must be 1..%d, got %d", who, MAX_SEG, E);
    MI355_REQUIRE(out_dtype == MI355_DT_BF16 || out_dtype == MI355_DT_F32, "%s: bad out_dtype", who);
    if (R <= 0) return 0;
    MI355_REQUIRE(M > 0 && N > 0, "%s: empty problem M=%ld N=%ld", who, (long)M, (long)N);
    MI355_REQUIRE(counts && offsets && A && B && C, "%s: null operand", who);
    MI355_REQUIRE((lda & 7) == 0 && (ldb & 7) == 0 && (ldc & 7) == 0 && (strideC & 7) == 0, "%s: lda / ldb / ldc / strideC must be multiples of 8", who);
    MI355_REQUIRE((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0, "%s: A / B / C must be 16-byte aligned", who);
    MI355_REQUIRE((M & 7) == 0 && (N & 7) == 0, "%s: M, N must be multiples of 8", who);
    MI355_REQUIRE(lda >= M && ldb >= N && ldc >= N && strideC >= (M - 1) * ldc + N, "%s: a pitch is shorter than its row, or the experts' outputs overlap", who);
    MI355_REQUIRE(lda * 2 * 256 < 0x7fffffffLL && ldb * 2 * 256 < 0x7fffffffLL && R < 0x7fffffffLL, "%s: leading dimension or R too large", who);
    MI355_REQUIRE(tile_hint == 0 || tile_hint == 1, "%s: tile_hint must be 0 (auto) or 1 (128x128)", who);
    if (residual) MI355_REQUIRE((ldr & 7) == 0 && ldr >= N && ((uintptr_t)residual & 15) == 0, "%s: residual rows must be 16-byte aligned and hold N columns", who);
    SegParams sp;
    seg_params_init(sp, E, counts, offsets, R, strideC);
    GemmParams& p = sp.p;
    p.A = (const bf16_t*)A; p.B = (const bf16_t*)B; p.C = C; p.R = residual;
    p.M = M; p.N = N; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldr = residual ? ldr : 0;
    p.epilogue = MI355_EPI_NONE;
    return launch_segmented_tn<Cfg128>(sp, out_dtype, (hipStream_t)stream);
}
