// Rollout sampling (generate.py: sample_rows, generate_batched_rollouts; alignment/rlhf_grpo: batched_responses_collator).  Two kernels:
//   * sample_rows_kernel: temperature / top-k / top-p / min-p sampling of one token per logits row [B, V] (bf16 or fp32, any row pitch >= V) in ONE
//     launch, one workgroup of 1024 threads per row, with the per-token bookkeeping of a batched rollout folded into its last thread
//     (finished rows emit pad, the response column, the finished flags, the key-mask column, the count of rows still live);
//   * response_masks_kernel: the attention and reward masks of a batch of finished rollouts, integer only.
// How a row is filtered.  Every decision about WHICH tokens stay is taken on integers: the order-preserving 32-bit key of the logit (ties are exact),
// counts, and probability mass in 2^-40 fixed point, which LDS integer atomics add in any order to the same bits.  A radix select walks a 43-bit
// composite key -- 11 bits of a linear bucket of (max - x), which spreads a bell-shaped row over ~2 000 LDS counters instead of the dozen that the
// exponent bits of a float give, then the key's own bits 11 + 11 + 10 -- from the top: each pass histograms the digit of the elements that match the
// decided prefix (count and mass), a block scan finds the digit where the k-th element (top-k) or the mass p * S (top-p) falls.  The kept set is
// then {key > T} + the first r elements of {key == T} in index order (+ {e >= min_p} for min-p), and the draw is an index-ordered pass: kept mass per
// 512-element wave tile (per lane 8 adds, then a wave scan: a fixed order), the tiles summed in fp64 by one thread, the chosen tile rescanned.
// Passes over the row: max/min 1, select 3 (bf16) or 4 (fp32) per selection (top-p with top-k: two selections), ties 1 (only when a tie is cut), draw 1;
// all but the first hit L2.  fp32 arithmetic for the probabilities (e = exp((x - max) / temp); its sum S is only needed by top-p).
#include <math.h>

#include "rows_bf16.h"

namespace {

constexpr int SMP_THREADS = 1024, SMP_WAVES = 16, SMP_NB = 2048, SMP_TILE = 512, SMP_MAX_TILES = 2048, SMP_MAX_EOS = 8;
constexpr int64_t SMP_MAX_V = (int64_t)SMP_TILE * SMP_MAX_TILES;  // 1 048 576: one fp32 + one u32 per wave tile in LDS
constexpr double SMP_FIX = 1099511627776.0;                       // 2^40: e <= 1, so a row's mass stays below 2^60
enum { SMP_NONE = 0, SMP_TOP_K = 1, SMP_TOP_P = 2, SMP_MIN_P = 3 };

typedef unsigned long long u64;
#define ST(s) ((hipStream_t)(s))

struct EosList {
    int n;
    int64_t id[SMP_MAX_EOS];
};

struct SampleParams {
    int64_t V, ld;
    const void* logits;
    int is_f32, mode, top_k;
    float top_p, min_p, inv_temp;
    const float* uniforms;
    unsigned seed_lo, seed_hi, off_lo, off_hi;
    int64_t* next;
    // rollout bookkeeping (all optional)
    uint8_t* finished;
    EosList eos;
    int64_t pad_id;
    int64_t* responses;
    int64_t ldr;
    uint8_t* key_mask;
    int64_t ldm, col;
    int32_t* live;
};

struct Row {
    const bf16_t* pb;
    const float* pf;
    int64_t V;
    bool f32, vec;
};

struct Shared {
    unsigned cnt[SMP_NB];
    u64 mass[SMP_NB];
    float tmass[SMP_MAX_TILES];
    unsigned tties[SMP_MAX_TILES];
    u64 wtot[SMP_WAVES];
    float redf[2 * SMP_WAVES];
    long long last[SMP_WAVES];
    // the digit a pass settled on
    int sel_found;
    unsigned sel_digit, sel_eq;
    u64 sel_above, sel_eqmass;
    // the draw
    long long draw_tile, draw_last;
    double draw_base, draw_target;
};

// elements i0 .. i0 + 7 of the row as floats; returns how many of them exist (the others read as -inf)
__device__ __forceinline__ int load8(const Row& r, int64_t i0, float (&x)[8]) {
    const int64_t rem = r.V - i0;
    const int n = rem >= 8 ? 8 : (rem > 0 ? (int)rem : 0);
    if (n == 8 && r.vec) {
        if (r.f32) {
            const f32x4 a = *(const f32x4*)(r.pf + i0), b = *(const f32x4*)(r.pf + i0 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = a[e], x[4 + e] = b[e];
        } else {
            unpack8(*(const u32x4*)(r.pb + i0), x);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = e < n ? (r.f32 ? r.pf[i0 + e] : bf2f(r.pb[i0 + e])) : -INFINITY;
    }
    return n;
}

// f(index, value) for every element of the row: wave w takes the 512-element tiles w, w + 16, ..., a lane 8 consecutive elements
template <class F>
__device__ __forceinline__ void for_each_elem(const Row& row, F f) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t ntiles = (row.V + SMP_TILE - 1) / SMP_TILE;
    for (int64_t q = w; q < ntiles; q += SMP_WAVES) {
        float x[8];
        const int64_t i0 = q * SMP_TILE + lane * 8;
        const int n = load8(row, i0, x);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (e < n) f(i0 + e, x[e]);
    }
}

// order-preserving key: a > b as floats <=> key(a) > key(b) as unsigned; -0 is +0; a bf16 row keeps 16 bits (the low ones are constant per sign)
__device__ __forceinline__ unsigned order_key(float x, bool f32) {
    x = x + 0.0f;
    const unsigned b = __float_as_uint(x);
    const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return f32 ? k : (k & 0xffff0000u);
}
// the composite key: the linear bucket of (M - x) on top (monotone in x: subtraction, the product with c > 0 and the truncation all are), then the key
__device__ __forceinline__ u64 composite_key(float x, float M, float c, bool f32) {
    const float t = (M - x) * c;
    const unsigned b = (t < 2047.f) ? (unsigned)(int)t : 2047u;  // -inf and NaN land in the last bucket
    return ((u64)(2047u - b) << 32) | order_key(x, f32);
}
__device__ __forceinline__ float prob_e(float x, float M, float inv_temp) { return expf((x - M) * inv_temp); }
__device__ __forceinline__ u64 fix40(float e) { return (u64)((double)e * SMP_FIX); }

// inclusive prefix sum over the 1024 threads (ascending thread index) and the total; integers, so the order of the adds is immaterial
__device__ __forceinline__ u64 block_scan(u64 v, u64* wtot, u64& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    __syncthreads();
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    u64 base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < SMP_WAVES; ++i) {
        const u64 t = wtot[i];
        if (i < w) base += t;
        total += t;
    }
    return v + base;
}

struct Selected {
    bool found;     // by mass: false when the whole row's mass does not exceed the target (keep everything)
    unsigned key;   // T
    unsigned r, eq; // keep the first r of the eq elements whose key is T
};

// Radix select over the composite key, from the top.  by_mass false: the k-th largest element (k <= V).  by_mass true: the element at which the
// running mass, in descending key order and index order among equals, first exceeds top_p * S (S the row's whole mass, from the first pass).
__device__ Selected radix_select(const Row& row, Shared& sh, bool by_mass, unsigned k, float top_p, float M, float c, float inv_temp) {
    const int SHIFT[4] = {32, 21, 10, 0}, NBITS[4] = {11, 11, 11, 10};
    const int npass = row.f32 ? 4 : 3;  // a bf16 key has no bits below 16: the third pass (bits 20..10) ends on a single key
    u64 prefix = 0, acc = 0, target = 0;
    unsigned krem = k;
    Selected out = {true, 0u, 0u, 0u};
    for (int p = 0; p < npass; ++p) {
        const int s = SHIFT[p], nb = NBITS[p];
        for (int i = threadIdx.x; i < SMP_NB; i += SMP_THREADS) sh.cnt[i] = 0u, sh.mass[i] = 0ull;
        if (threadIdx.x == 0) sh.sel_found = 0;
        __syncthreads();
        for_each_elem(row, [&](int64_t, float x) {
            const u64 ck = composite_key(x, M, c, row.f32);
            if ((ck >> (s + nb)) == prefix) {
                const unsigned d = (unsigned)(ck >> s) & ((1u << nb) - 1u);
                atomicAdd(&sh.cnt[d], 1u);
                if (by_mass) atomicAdd(&sh.mass[d], fix40(prob_e(x, M, inv_temp)));
            }
        });
        __syncthreads();
        // descending digits: thread t holds digits hi = NB - 1 - 2 t and hi - 1
        const int hi = SMP_NB - 1 - 2 * (int)threadIdx.x;
        const u64 v0 = by_mass ? sh.mass[hi] : (u64)sh.cnt[hi], v1 = by_mass ? sh.mass[hi - 1] : (u64)sh.cnt[hi - 1];
        u64 total;
        const u64 incl = block_scan(v0 + v1, sh.wtot, total), excl = incl - (v0 + v1);
        if (by_mass && p == 0) target = (u64)((double)top_p * (double)total);
        int pick = -1;
        if (by_mass) {  // first digit whose inclusive running mass exceeds the target
            if (acc + excl <= target && acc + excl + v0 > target) pick = hi;
            else if (acc + excl + v0 <= target && acc + incl > target) pick = hi - 1;
        } else {  // first digit whose inclusive running count reaches krem
            if (excl < krem && excl + v0 >= krem) pick = hi;
            else if (excl + v0 < krem && incl >= krem) pick = hi - 1;
        }
        if (pick >= 0) {
            sh.sel_found = 1;
            sh.sel_digit = (unsigned)pick;
            sh.sel_above = pick == hi ? excl : excl + v0;
            sh.sel_eq = sh.cnt[pick];
            sh.sel_eqmass = sh.mass[pick];
        }
        __syncthreads();
        if (!sh.sel_found) {  // by mass, first pass: the row's mass does not exceed p * S (p >= 1)
            out.found = false;
            __syncthreads();
            return out;
        }
        prefix = (prefix << nb) | sh.sel_digit;
        if (by_mass) acc += sh.sel_above;
        else krem -= (unsigned)sh.sel_above;
        if (p == npass - 1) {
            out.key = (unsigned)(prefix << s);
            out.eq = sh.sel_eq;
            if (by_mass) {  // the eq tied elements carry the same mass f each: the r-th of them crosses
                const u64 f = sh.sel_eqmass / (u64)sh.sel_eq;
                const u64 r = f ? (target - acc) / f + 1ull : (u64)sh.sel_eq;
                out.r = r < (u64)sh.sel_eq ? (unsigned)r : sh.sel_eq;
            } else {
                out.r = krem;
            }
        }
        __syncthreads();  // the sel_* words are read: the next pass may reset them
    }
    return out;
}

struct Keep {
    unsigned T, r;
    bool all_ties, minp;
    float min_p;
};

// One wave tile: the kept mass of each of this lane's 8 elements (0 where the token is dropped), their sum, and the lane's first element index.
// tie_base[q]: how many elements with key == T precede tile q (read only when a tie is cut).
__device__ __forceinline__ float tile_eval(const Row& row, int64_t q, const Keep& kp, float M, float inv_temp, const unsigned* tie_base, float (&km)[8],
                                           int64_t& i0, long long& lastpos) {
    const int lane = threadIdx.x & 63;
    float x[8];
    i0 = q * SMP_TILE + lane * 8;
    const int n = load8(row, i0, x);
    unsigned key[8];
    unsigned tc = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        key[e] = order_key(x[e], row.f32);
        tc += (e < n && key[e] == kp.T) ? 1u : 0u;
    }
    unsigned rank = 0;
    if (!kp.all_ties) {
        unsigned inc = tc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        rank = tie_base[q] + inc - tc;
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        bool keep = false;
        float ev = 0.f;
        if (e < n) {
            ev = prob_e(x[e], M, inv_temp);
            if (key[e] > kp.T) keep = true;
            else if (key[e] == kp.T) {
                keep = kp.all_ties || rank < kp.r;
                ++rank;
            }
            if (kp.minp && ev >= kp.min_p) keep = true;
        }
        km[e] = keep ? ev : 0.f;
        s += km[e];
        if (km[e] > 0.f) lastpos = i0 + e;
    }
    return s;
}

__device__ __forceinline__ float wave_scan_f32(float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// the rollout's bookkeeping for row b and the sampled token (generate.py's loop body, reference :341-350), by one thread
__device__ void finish_row(const SampleParams& P, int64_t b, int64_t sampled) {
    uint8_t fin = P.finished ? P.finished[b] : (uint8_t)0;
    const int64_t tok = fin ? P.pad_id : sampled;
    P.next[b] = tok;
    if (P.responses) P.responses[b * P.ldr + P.col] = tok;
    if (P.finished) {
        for (int i = 0; i < P.eos.n; ++i) fin |= (tok == P.eos.id[i]) ? 1 : 0;
        P.finished[b] = fin ? 1 : 0;
        if (P.key_mask) P.key_mask[b * P.ldm + P.col] = fin ? 0 : 1;
        if (P.live && !fin) atomicAdd(P.live, 1);
    }
}

__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(const SampleParams P) {
    __shared__ Shared sh;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (P.finished && P.finished[b]) {  // a finished row emits pad whatever its logits say
        if (threadIdx.x == 0) finish_row(P, b, P.pad_id);
        return;
    }
    Row row;
    row.V = P.V;
    row.f32 = P.is_f32 != 0;
    row.pb = (const bf16_t*)P.logits + b * P.ld;
    row.pf = (const float*)P.logits + b * P.ld;
    row.vec = ((row.f32 ? (uintptr_t)row.pf : (uintptr_t)row.pb) & 15) == 0;

    // ---- the row's maximum and its smallest finite value
    float mx = -INFINITY, mn = INFINITY;
    for_each_elem(row, [&](int64_t, float x) {
        mx = fmaxf(mx, x);
        if (x > -INFINITY) mn = fminf(mn, x);
    });
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if (lane == 0) sh.redf[w] = mx, sh.redf[SMP_WAVES + w] = mn;
    __syncthreads();
    float M = sh.redf[0];
    mn = sh.redf[SMP_WAVES];
#pragma unroll
    for (int i = 1; i < SMP_WAVES; ++i) M = fmaxf(M, sh.redf[i]), mn = fminf(mn, sh.redf[SMP_WAVES + i]);
    const float c = (M > mn && M < INFINITY) ? 2047.f / (M - mn) : 0.f;
    __syncthreads();

    // ---- which tokens stay
    Keep kp = {0u, 0u, true, false, 0.f};
    if (P.mode == SMP_TOP_K) {
        const Selected s = radix_select(row, sh, false, (unsigned)P.top_k, 0.f, M, c, P.inv_temp);
        kp.T = s.key, kp.r = s.r, kp.all_ties = s.r == s.eq;
    } else if (P.mode == SMP_TOP_P) {
        unsigned Tk = 0u;
        if (P.top_k > 0) Tk = radix_select(row, sh, false, (unsigned)P.top_k, 0.f, M, c, P.inv_temp).key;  // every tie at the k-th value stays
        const Selected s = radix_select(row, sh, true, 0u, P.top_p, M, c, P.inv_temp);
        if (s.found && s.key >= Tk) kp.T = s.key, kp.r = s.r, kp.all_ties = s.r == s.eq;
        else kp.T = Tk;
    } else if (P.mode == SMP_MIN_P) {
        const Selected s = radix_select(row, sh, false, (unsigned)(P.top_k > 0 ? P.top_k : 1), 0.f, M, c, P.inv_temp);
        kp.T = s.key, kp.r = s.r, kp.all_ties = s.r == s.eq;
        kp.minp = true, kp.min_p = P.min_p;  // p_i >= min_p * p_max with e_max = exp(0) = 1
    }
    const int64_t ntiles = (row.V + SMP_TILE - 1) / SMP_TILE;

    // ---- a cut tie: the rank of every tied element in index order
    if (!kp.all_ties) {
        for (int64_t q = w; q < ntiles; q += SMP_WAVES) {
            float x[8];
            const int n = load8(row, q * SMP_TILE + lane * 8, x);
            unsigned tc = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) tc += (e < n && order_key(x[e], row.f32) == kp.T) ? 1u : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) tc += __shfl_xor(tc, o, 64);
            if (lane == 0) sh.tties[q] = tc;
        }
        __syncthreads();
        const int64_t q0 = 2 * (int64_t)threadIdx.x;
        const unsigned a0 = q0 < ntiles ? sh.tties[q0] : 0u, a1 = q0 + 1 < ntiles ? sh.tties[q0 + 1] : 0u;
        u64 total;
        const u64 incl = block_scan((u64)a0 + a1, sh.wtot, total);
        if (q0 < ntiles) sh.tties[q0] = (unsigned)(incl - a0 - a1);
        if (q0 + 1 < ntiles) sh.tties[q0 + 1] = (unsigned)(incl - a1);
        __syncthreads();
    }

    // ---- the kept mass of every wave tile, in index order
    long long lastpos = -1;
    for (int64_t q = w; q < ntiles; q += SMP_WAVES) {
        float km[8];
        int64_t i0;
        const float s = tile_eval(row, q, kp, M, P.inv_temp, sh.tties, km, i0, lastpos);
        const float incl = wave_scan_f32(s);
        if (lane == 63) sh.tmass[q] = incl;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long t = __shfl_xor(lastpos, o, 64);
        lastpos = t > lastpos ? t : lastpos;
    }
    if (lane == 0) sh.last[w] = lastpos;
    __syncthreads();

    // ---- the draw: u * Z against the running sum of the tiles, fp64, one thread
    if (threadIdx.x == 0) {
        float u;
        if (P.uniforms) {
            u = P.uniforms[b];
        } else {
            unsigned r4[4];
            philox4x32_10((unsigned)b, 0u, P.off_lo, P.off_hi, P.seed_lo, P.seed_hi, r4);
            u = (float)(r4[0] >> 8) * 5.9604644775390625e-8f;  // 2^-24
        }
        double Z = 0.0;
        for (int64_t q = 0; q < ntiles; ++q) Z += (double)sh.tmass[q];
        const double target = (double)u * Z;
        double cum = 0.0, base = 0.0;
        long long sel = -1;
        for (int64_t q = 0; q < ntiles; ++q) {
            const double nc = cum + (double)sh.tmass[q];
            if (sel < 0 && nc > target) sel = q, base = cum;
            cum = nc;
        }
        long long last = -1;
        for (int i = 0; i < SMP_WAVES; ++i) last = sh.last[i] > last ? sh.last[i] : last;
        sh.draw_tile = sel, sh.draw_base = base, sh.draw_target = target, sh.draw_last = last < 0 ? 0 : last;
    }
    __syncthreads();
    if (w != 0) return;
    long long tok = sh.draw_last;  // rounding left no crossing: the last kept token
    if (sh.draw_tile >= 0) {
        float km[8];
        int64_t i0;
        long long lp = -1;
        const float s = tile_eval(row, sh.draw_tile, kp, M, P.inv_temp, sh.tties, km, i0, lp);
        const float incl = wave_scan_f32(s);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.f;
        const double base = sh.draw_base, target = sh.draw_target;
        const u64 cross = __ballot(base + (double)incl > target);
        if (cross) {
            const int Lc = __ffsll((long long)cross) - 1;
            long long mine = -1, lastk = -1;
            float run = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (km[e] > 0.f) {
                    run += km[e];
                    lastk = i0 + e;
                    if (mine < 0 && base + (double)excl + (double)run > target) mine = i0 + e;
                }
            }
            if (mine < 0) mine = lastk;
            mine = __shfl(mine, Lc, 64);
            if (mine >= 0) tok = mine;
        }
    }
    if (lane == 0) finish_row(P, b, tok);
}

// batched_responses_collator (reference grpo_engine.py:325-345): stop = (EOS or pad) at a column >= P; attended while the running count of stops is <= 1,
// that is before the SECOND stop column (a rollout is all pad after its first stop, so its first stop is its last attended column); the prompt columns
// take prompt_masks; the reward mask is the attention mask without the prompt.  One wave per row.
__device__ __forceinline__ bool is_stop(int64_t tok, const EosList& eos, int64_t pad) {
    bool s = tok == pad;
    for (int i = 0; i < eos.n; ++i) s |= tok == eos.id[i];
    return s;
}
__device__ __forceinline__ long long wave_min_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__global__ __launch_bounds__(64) void response_masks_kernel(int64_t S, int64_t P, const int64_t* __restrict__ resp, int64_t ldr, const uint8_t* __restrict__ pm,
                                                            int64_t ldp, const EosList eos, int64_t pad, uint8_t* __restrict__ attn, uint8_t* __restrict__ reward) {
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t* r = resp + b * ldr;
    long long f1 = S, f2 = S;
    for (int64_t s = P + lane; s < S; s += 64)
        if (is_stop(r[s], eos, pad)) {
            f1 = s;
            break;
        }
    f1 = wave_min_ll(f1);
    for (int64_t s = P + lane; s < S; s += 64)
        if (s > f1 && is_stop(r[s], eos, pad)) {
            f2 = s;
            break;
        }
    f2 = wave_min_ll(f2);
    for (int64_t s = lane; s < S; s += 64) {
        const bool a = s < P ? pm[b * ldp + s] != 0 : s < f2;
        attn[b * S + s] = a ? 1 : 0;
        reward[b * S + s] = (s >= P && a) ? 1 : 0;
    }
}

int fill_eos(EosList& e, const int64_t* eos_ids, int n_eos) {
    e.n = n_eos;
    for (int i = 0; i < SMP_MAX_EOS; ++i) e.id[i] = i < n_eos ? eos_ids[i] : 0;
    return 0;
}

}  // namespace

extern "C" int mi355_sample_rows(int64_t B, int64_t V, const void* logits, int dtype, int64_t ld, int mode, int top_k, float top_p, float min_p, float temp,
                                 const float* uniforms, uint64_t seed, uint64_t offset, int64_t* next, uint8_t* finished, const int64_t* eos_ids, int n_eos,
                                 int64_t pad_id, int64_t* responses, int64_t ldr, uint8_t* key_mask, int64_t ldm, int64_t col, int32_t* live, void* stream) {
    MI355_REQUIRE(B > 0 && B <= 65535 && V > 0 && V <= SMP_MAX_V, "sample_rows: 1 <= B <= 65535 rows of 1 <= V <= %lld logits (got B %lld, V %lld)",
                  (long long)SMP_MAX_V, (long long)B, (long long)V);
    MI355_REQUIRE(logits && next && ld >= V, "sample_rows: null logits / output, or a row pitch below V");
    MI355_REQUIRE(dtype == MI355_DT_BF16 || dtype == MI355_DT_F32, "sample_rows: logits must be bf16 (0) or fp32 (1), got dtype %d", dtype);
    MI355_REQUIRE(mode >= SMP_NONE && mode <= SMP_MIN_P, "sample_rows: mode %d (0 none, 1 top-k, 2 top-p, 3 min-p)", mode);
    MI355_REQUIRE(temp > 0.f && temp < INFINITY, "sample_rows: the temperature must be positive and finite (greedy decoding is mi355_argmax_rows)");
    MI355_REQUIRE(top_k >= 0 && top_k <= V && (mode != SMP_TOP_K || top_k >= 1), "sample_rows: top_k %d outside 1..V (0: none, modes 2 and 3 only)", top_k);
    MI355_REQUIRE(mode != SMP_TOP_P || (top_p > 0.f && top_p < INFINITY), "sample_rows: top_p must be positive");
    MI355_REQUIRE(mode != SMP_MIN_P || (min_p > 0.f && min_p <= 1.f), "sample_rows: min_p must lie in (0, 1]");
    MI355_REQUIRE(n_eos >= 0 && n_eos <= SMP_MAX_EOS && (n_eos == 0 || eos_ids), "sample_rows: 0..%d EOS ids (a host array)", SMP_MAX_EOS);
    MI355_REQUIRE(finished || (!key_mask && !live && n_eos == 0), "sample_rows: the key mask, the live count and the EOS ids need the finished flags");
    MI355_REQUIRE(!responses || (col >= 0 && col < ldr), "sample_rows: the response column lies outside the row pitch");
    MI355_REQUIRE(!key_mask || (col >= 0 && col < ldm), "sample_rows: the key-mask column lies outside the row pitch");
    SampleParams P;
    P.V = V, P.ld = ld, P.logits = logits, P.is_f32 = dtype == MI355_DT_F32, P.mode = mode, P.top_k = top_k;
    P.top_p = top_p, P.min_p = min_p, P.inv_temp = 1.0f / temp, P.uniforms = uniforms;
    P.seed_lo = (unsigned)seed, P.seed_hi = (unsigned)(seed >> 32), P.off_lo = (unsigned)offset, P.off_hi = (unsigned)(offset >> 32);
    P.next = next, P.finished = finished, P.pad_id = pad_id, P.responses = responses, P.ldr = ldr, P.key_mask = key_mask, P.ldm = ldm, P.col = col, P.live = live;
    fill_eos(P.eos, eos_ids, n_eos);
    sample_rows_kernel<<<(unsigned)B, SMP_THREADS, 0, ST(stream)>>>(P);
    MI355_LAUNCH_CHECK("sample_rows");
    return 0;
}

extern "C" int mi355_response_masks(int64_t B, int64_t S, int64_t P, const int64_t* responses, int64_t ldr, const uint8_t* prompt_masks, int64_t ldp,
                                    const int64_t* eos_ids, int n_eos, int64_t pad_id, uint8_t* attn_masks, uint8_t* reward_masks, void* stream) {
    MI355_REQUIRE(B > 0 && B <= 65535 && S > 0 && P >= 0 && P <= S, "response_masks: 1 <= B <= 65535 rows of S >= 1 columns, 0 <= P <= S");
    MI355_REQUIRE(responses && attn_masks && reward_masks && ldr >= S && (P == 0 || (prompt_masks && ldp >= P)), "response_masks: null pointer or a pitch below the row");
    MI355_REQUIRE(n_eos >= 0 && n_eos <= SMP_MAX_EOS && (n_eos == 0 || eos_ids), "response_masks: 0..%d EOS ids (a host array)", SMP_MAX_EOS);
    EosList e;
    fill_eos(e, eos_ids, n_eos);
    response_masks_kernel<<<(unsigned)B, 64, 0, ST(stream)>>>(S, P, responses, ldr, prompt_masks, ldp, e, pad_id, attn_masks, reward_masks);
    MI355_LAUNCH_CHECK("response_masks");
    return 0;
}
