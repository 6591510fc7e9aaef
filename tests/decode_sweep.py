"""The fp64 sweep of the decode kernels (csrc/decode.hip): case tables, operand builders, fp64 references, an fp32 emulation of the attention
kernel's order of operations, and the judgement shared by test_decode_sweep_gpu.py and test_decode_sweep_cpu.py.  TEST INFRASTRUCTURE ONLY.

Geometry.  ``attn_decode`` deals chunks of CK keys to 8 waves and S splits: chunk c goes to split c % S, there to wave (c / S) % 8, in trip
c / (8 S) of that wave's key loop; inside a chunk key j sits in slot t = (j % CK) / KG of key group j % KG.  ``GEOMETRY`` states KG, NT and CK per head
dim ONCE; every length, needle position and coverage claim below is derived from it (``place``).

Operands.  The caches are views into larger storages (row pitch Hkv D + 8, batch stride (capacity + 3) rows); every element the kernel has no business
reading -- rows at or past the effective length, the pitch slack, the rows between the samples -- holds bf16 NaN, mask bytes past the effective length
are 0, and the fp64 reference reads the visible part only.

Judgement of the attention context (``judge``), per (sample, head) and element by element:
    |o - ref64| <= 2^-7 |ref64| + c * sum_j p_j |v_j|.
The first term is the bf16 rounding of the output (half an ulp is at most 2^-8 relative; doubled because the rounded value is itself an fp32 result).
c covers the fp32 arithmetic in front of that rounding and is MEASURED per case (``measure_c``): the largest |ref32 - ref64| / sum p |v| of a plain
fp32 torch evaluation of the same formula, times 64 (the kernel sums in another order, works in the log2 domain with the scale folded into one fp32
constant and uses the hardware exp2), with a floor of 2^-20 and a cap of 2^-10.  The cap is a condition on the case, not a bound that is widened: a
case whose fp32 reference alone needs more is a wrong case for this test, and the CPU test asserts the cap for every case.  Measured (the figure depends
on the host's fp32 matmul, two hosts are quoted): over the 40 grid cases c runs from the floor, 9.5e-7 (one-key cases: the fp32 reference is exact), to
3.5e-5, over the peaked cases from 5.1e-5 to 1.2e-4 (D = 256); the cap is 9.8e-4.  For ``gemv`` (same rule, sum_k |x| |w| + |r| in place of
sum p |v|) c runs from the floor to 3.1e-6.  With c this small the bound is the output's bf16 rounding almost everywhere: the emulation and the
kernel both use about half of it (largest error / bound 0.50).
A NaN or Inf anywhere in an output fails the case by (sample, head).  No (sample, head) is left out: ``judge`` returns how many it judged.

Needle cases.  One key per sample is 8 q of its head (rounded to bf16): it leads every other score by more than 30 nats, the other keys' total weight
is below 2^-24, exp2(0) is exactly 1, and the context must equal that key's value row bit for bit.  The positions are the chunk and round edges
(``needle_positions``) plus a diagonal that puts a needle into every key group, every slot, every wave and the first two trips.
"""

import math
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

BF16 = torch.bfloat16
WAVES = 8
# D: (KG key groups = keys per load instruction, NT keys per lane and chunk, CK = NT * KG keys per chunk)  -- csrc/decode.hip, attn_decode_kernel
GEOMETRY = {32: (16, 4, 64), 64: (8, 8, 64), 128: (4, 8, 32), 256: (2, 8, 16)}
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
MASK_T = -2.0e38  # the kernel's finite fill, log2 domain
FILL = MASK_T * LN2  # the same fill in natural-log units (fp32-finite)
C_FLOOR, C_CAP, C_FACTOR = 2.0 ** -20, 2.0 ** -10, 64.0
OUT_ROUNDING = 2.0 ** -7

HEADS = ((1, 1), (4, 2), (8, 2), (6, 3), (5, 1))  # Hq, Hkv
SPLITS = (1, 2, 3, 7, 64)
SOURCES = ("host", "dev_equal", "dev_shorter", "dev_longer")  # where the effective length comes from
MASKS = ("none", "holes", "chunk", "sample1")
BATCH = 2
MARGIN = 5  # capacity = length + MARGIN rows

AttnCase = namedtuple("AttnCase", "name D L Hq Hkv splits source mask scale order")


def geometry(D):
    KG, NT, CK = GEOMETRY[D]
    assert KG * (D // 8) == 64 and CK == NT * KG and NT == min(D // 8, 8)
    return KG, NT, CK, WAVES * CK


def longest(D):
    KG, NT, CK, ROUND = geometry(D)
    return 2 * ROUND + CK + KG + 1


def lengths(D):
    KG, NT, CK, ROUND = geometry(D)
    return (1, KG, KG + 1, CK - 1, CK, CK + 1, ROUND - 1, ROUND, ROUND + 1, longest(D))


def place(D, j, S):
    """Where the kernel puts key j under S splits -> dict(kg, t, chunk, split, wave, trip)."""
    KG, NT, CK, ROUND = geometry(D)
    c = j // CK
    return {"kg": j % KG, "t": (j % CK) // KG, "chunk": c, "split": c % S, "wave": (c // S) % WAVES, "trip": c // (S * WAVES)}


def n_chunks(D, L):
    return (L + GEOMETRY[D][2] - 1) // GEOMETRY[D][2]


def grid_cases():
    """The 40 cases: per head dim its ten lengths; heads, splits, length source and mask kind rotate with the length index so that every value of each
    meets every D (test_decode_sweep_cpu.py asserts it)."""
    out = []
    for di, D in enumerate(GEOMETRY):
        for li, L in enumerate(lengths(D)):
            Hq, Hkv = HEADS[(li + di) % 5]
            # (the steps are chosen so that, per D, one case each has: a masked chunk beside visible ones, a second trip of the key loop, a split
            # without keys, several splits that all own keys, a device-side length shorter than a capacity of several chunks)
            S = SPLITS[(2 * li + 2) % 5]
            src = SOURCES[(li + di + 3 * (li // 4)) % 4]
            mask = MASKS[(li + li // 4 + 2) % 4]
            out.append(AttnCase(f"D{D}-L{L}-H{Hq}x{Hkv}-S{S}-{src}-{mask}", D, L, Hq, Hkv, S, src, mask, None, None))
    return out


def peaked_cases():
    """One per D, each at splits 1 and 3: the longest length, scale 4 / sqrt(D), the keys sorted by head 0's score -- ascending in sample 0 (the running
    maximum moves in every chunk), descending in sample 1."""
    return [AttnCase(f"peaked-D{D}-S{S}", D, longest(D), 4, 2, S, "host", "none", 4.0 / math.sqrt(D), "sorted") for D in GEOMETRY for S in (1, 3)]


WIDE_CASE = AttnCase("D128-L300-H16x8-S1-host-none", 128, 300, 16, 8, 1, "host", "none", None, None)  # 16 heads: what a per-head judgement adds


def _nan_storage(n):
    return torch.full((n,), float("nan"), dtype=BF16)


def cache_view(storage, B, cap, width, ld):
    """[B, cap, width] with row pitch ld and batch stride (cap + 3) * ld into a 1-D storage"""
    return storage.as_strided((B, cap, width), ((cap + 3) * ld, ld, 1))


def _caches(B, cap, width):
    ld = width + 8
    n = B * (cap + 3) * ld
    ks, vs = _nan_storage(n), _nan_storage(n)
    return ks, vs, ld


def _mask(kind, D, B, L, cap):
    """-> (uint8 [B, cap + 7] whose first ``cap`` columns are the mask the kernel gets, bool [B, L] of visible keys) or (None, all True)"""
    vis = torch.ones(B, L, dtype=torch.bool)
    if kind == "none":
        return None, vis
    CK = GEOMETRY[D][2]
    j = torch.arange(L)
    if kind == "holes":  # every visible byte value the reference's ``bool`` mask can arrive as
        for b in range(B):
            vis[b] = (j % (5 + 2 * b)) != 2
    elif kind == "chunk":  # sample 0: the first chunk, the last sample: the last (ragged) chunk -- a wave whose running maximum is the fill
        vis[0, :CK] = False
        last = (L - 1) // CK
        vis[B - 1, last * CK :] = False
    elif kind == "sample1":  # finite fill: uniform attention over the cache
        vis[1] = False
    else:
        raise ValueError(kind)
    wide = torch.zeros(B, cap + 7, dtype=torch.uint8)
    byte = torch.tensor([1, 2, 255], dtype=torch.uint8)[j % 3] if kind == "holes" else torch.ones(L, dtype=torch.uint8)
    wide[:, :L] = byte[None, :] * vis.to(torch.uint8)
    return wide, vis


@lru_cache(maxsize=None)
def build(case):
    """CPU operands of one attention case -> namespace(q [B, Hq D]; ks, vs storages; ld, cap; km_wide or None; vis bool [B, L]; L effective, host_len,
    len_dev int or None; scale float)."""
    D, L, Hq, Hkv = case.D, case.L, case.Hq, case.Hkv
    B, cap = BATCH, L + MARGIN
    g = torch.Generator().manual_seed(1000 * D + 7 * L + Hq)
    q = torch.randn(B, Hq * D, generator=g).to(BF16)
    k = torch.randn(B, L, Hkv * D, generator=g).to(BF16)
    v = torch.randn(B, L, Hkv * D, generator=g).to(BF16)
    if case.order == "sorted":
        s0 = torch.einsum("bd,bld->bl", q[:, :D].double(), k[:, :, :D].double())
        for b in range(B):
            k[b] = k[b, torch.argsort(s0[b], descending=b % 2 == 1)]
    ks, vs, ld = _caches(B, cap, Hkv * D)
    cache_view(ks, B, cap, Hkv * D, ld)[:, :L] = k
    cache_view(vs, B, cap, Hkv * D, ld)[:, :L] = v
    km_wide, vis = _mask(case.mask, D, B, L, cap)
    host_len, len_dev = {"host": (L, None), "dev_equal": (L, L), "dev_shorter": (cap, L), "dev_longer": (L, L + 3)}[case.source]
    return SimpleNamespace(q=q, ks=ks, vs=vs, ld=ld, cap=cap, km_wide=km_wide, vis=vis, L=L, host_len=host_len, len_dev=len_dev,
                           scale=D ** -0.5 if case.scale is None else case.scale, B=B, Hq=Hq, Hkv=Hkv, D=D)


def views(ns, device="cpu"):
    """-> q, kc, vc, key mask (or None) on ``device``, laid out as ``build`` describes"""
    width = ns.Hkv * ns.D
    kc = cache_view(ns.ks.to(device), ns.B, ns.cap, width, ns.ld)
    vc = cache_view(ns.vs.to(device), ns.B, ns.cap, width, ns.ld)
    km = None if ns.km_wide is None else ns.km_wide.to(device)[:, : ns.cap]
    return ns.q.to(device), kc, vc, km


# ----------------------------------------------------------------------------------------------------------------- references
def softmax_reference(ns, dtype):
    """Plain evaluation in ``dtype`` on the visible keys only -> (o, sum_j p_j |v_j|, scores), o and the sum [B, Hq, D]"""
    B, Hq, Hkv, D, L = ns.B, ns.Hq, ns.Hkv, ns.D, ns.L
    _, kc, vc, _ = views(ns)
    src = torch.arange(Hq) // (Hq // Hkv)
    q = ns.q.to(dtype).view(B, Hq, D)
    k = kc[:, :L].to(dtype).view(B, L, Hkv, D)[:, :, src]
    v = vc[:, :L].to(dtype).view(B, L, Hkv, D)[:, :, src]
    s = torch.einsum("bhd,blhd->bhl", q, k) * ns.scale
    s = s.masked_fill(~ns.vis[:, None, :], FILL)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhl,blhd->bhd", p, v), torch.einsum("bhl,blhd->bhd", p, v.abs()), s


def measure_c(ref32, ref64, weight):
    """-> (64 x the fp32 reference's largest error per unit of ``weight``, the c of the bound: that figure under the floor)."""
    raw = C_FACTOR * float(((ref32.double() - ref64).abs() / weight.clamp_min(1e-300)).max())
    return raw, max(raw, C_FLOOR)


@lru_cache(maxsize=None)
def exact(case):
    """-> namespace(ref fp64 [B, Hq, D], weight = sum p |v| fp64, c_raw, c) of a case, computed once per process"""
    ns = build(case)
    o64, w64, _ = softmax_reference(ns, torch.float64)
    o32, _, _ = softmax_reference(ns, torch.float32)
    raw, c = measure_c(o32, o64, w64)
    return SimpleNamespace(ref=o64, weight=w64, c_raw=raw, c=c)


def judge(got, ex, label):
    """got bf16 [B, Hq * D] -> ((sample, head) pairs judged, failure strings naming sample and head, largest error / bound over the finite elements)"""
    B, Hq, D = ex.ref.shape
    o = got.detach().cpu().double().view(B, Hq, D)
    bound = OUT_ROUNDING * ex.ref.abs() + ex.c * ex.weight
    judged, fails, worst = 0, [], 0.0
    for b in range(B):
        for h in range(Hq):
            judged += 1
            if not bool(torch.isfinite(o[b, h]).all()):
                d = int((~torch.isfinite(o[b, h])).nonzero()[0])
                fails.append(f"{label}: sample {b}, head {h}: not finite at feature {d}")
                continue
            over = (o[b, h] - ex.ref[b, h]).abs() - bound[b, h]
            worst = max(worst, float(((o[b, h] - ex.ref[b, h]).abs() / bound[b, h]).max()))
            if bool((over > 0).any()):
                d = int(over.argmax())
                fails.append(f"{label}: sample {b}, head {h}, feature {d}: |{float(o[b, h, d]):.6e} - {float(ex.ref[b, h, d]):.6e}| > "
                             f"{float(bound[b, h, d]):.3e} (c = {ex.c:.2e}; {int((over > 0).sum())} of {D} features)")
    return judged, fails, worst


def report(label, ex, worst=None):
    print(f"[decode sweep] {label}: c = {ex.c:.3e} (64 x fp32 reference error {ex.c_raw:.3e})" + ("" if worst is None else f", largest error / bound {worst:.3f}"))


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def bits(t):
    """bf16 -> int16 view: comparisons that see NaN payloads"""
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


# ----------------------------------------------------------------------------------------------------------------- the emulation
DEFECTS = ("drop_last_key", "swap_values", "skip_wave", "empty_split_weight_1", "scale_head", "nan_past_len")


def emulate(ns, splits, defect=None):
    """The kernel's order of operations in fp32 on the operands of ``build``: log2-domain scores with the scale folded into one fp32 constant, zero
    rows and -inf scores past the length, the online softmax chunk by chunk in the kernel's assignment of chunks to splits and waves, the wave fold,
    the split fold, one bf16 rounding.  -> bf16 [B, Hq * D].

    ``defect`` (CPU only: what the judgement must catch) -- drop_last_key: key L - 1 is not attended; swap_values: value rows 0 and 1 of chunk 0 change
    places; skip_wave: wave 0 of split 0 is left out of the wave fold; empty_split_weight_1: the first split without keys enters the split fold with
    weight 1 and a sum of 1 (one phantom key at the maximum with a zero value row); scale_head: head 5 of sample 0 times 1.01 in front of the
    rounding; nan_past_len: the row at index L is read as if it were visible."""
    assert defect is None or defect in DEFECTS
    B, Hq, Hkv, D, L, S = ns.B, ns.Hq, ns.Hkv, ns.D, ns.L, splits
    KG, NT, CK, ROUND = geometry(D)
    f32 = torch.float32
    _, kc, vc, km = views(ns)
    src = torch.arange(Hq) // (Hq // Hkv)
    q = ns.q.float().view(B, Hq, D)
    scale_log2 = torch.tensor(ns.scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    length = min(ns.host_len, ns.len_dev) if ns.len_dev is not None else ns.host_len
    assert length == L
    if defect == "drop_last_key":
        length = L - 1
    elif defect == "nan_past_len":
        length = L + 1
    ninf = torch.full((B, Hq), -math.inf, dtype=f32)
    split_m, split_l, split_o = [], [], []
    for sp in range(S):
        wm, wl, wo = [], [], []
        for w in range(WAVES):
            m, l, acc = ninf.clone(), torch.zeros(B, Hq, dtype=f32), torch.zeros(B, Hq, D, dtype=f32)
            c = sp + S * w
            while c * CK < length:
                j0, j1 = c * CK, min(c * CK + CK, length)
                k = kc[:, j0:j1].float().view(B, j1 - j0, Hkv, D)[:, :, src]
                v = vc[:, j0:j1].float().view(B, j1 - j0, Hkv, D)[:, :, src]
                if defect == "swap_values" and c == 0:
                    assert j1 - j0 >= 2
                    v = torch.cat([v[:, 1:2], v[:, 0:1], v[:, 2:]], dim=1)
                sc = torch.einsum("bhd,bnhd->bhn", q, k) * scale_log2
                if km is not None:
                    sc = torch.where((km[:, j0:j1] == 0)[:, None, :], torch.tensor(MASK_T, dtype=f32), sc)
                mn = torch.maximum(m, sc.max(dim=-1).values)
                alpha = torch.exp2(m - mn)  # m = -inf on the first chunk -> 0
                p = torch.exp2(sc - mn[..., None])
                l = l * alpha + p.sum(dim=-1)
                acc = acc * alpha[..., None] + torch.einsum("bhn,bnhd->bhd", p, v)
                m = mn
                c += S * WAVES
            if defect == "skip_wave" and sp == 0 and w == 0:
                m, l, acc = ninf.clone(), torch.zeros_like(l), torch.zeros_like(acc)
            wm.append(m), wl.append(l), wo.append(acc)
        mg = torch.stack(wm).max(dim=0).values
        lg, out = torch.zeros(B, Hq, dtype=f32), torch.zeros(B, Hq, D, dtype=f32)
        for m, l, acc in zip(wm, wl, wo):
            f = torch.where(m == -math.inf, torch.zeros_like(m), torch.exp2(m - mg))
            lg = lg + l * f
            out = out + acc * f[..., None]
        split_m.append(mg), split_l.append(lg), split_o.append(out)
    if S == 1:
        lg, out = split_l[0], split_o[0]
    else:
        mg = torch.stack(split_m).max(dim=0).values
        lg, out = torch.zeros(B, Hq, dtype=f32), torch.zeros(B, Hq, D, dtype=f32)
        phantom = defect == "empty_split_weight_1"
        for m, l, acc in zip(split_m, split_l, split_o):
            empty = m == -math.inf
            f = torch.where(empty, torch.zeros_like(m), torch.exp2(m - mg))
            if phantom and bool(empty.all()):
                f, l, phantom = torch.ones_like(m), torch.ones_like(l), False
            lg = lg + l * f
            out = out + acc * f[..., None]
        assert not phantom, "the case has no empty split"
    o = out / lg[..., None]
    if defect == "scale_head":
        o[0, 5] = o[0, 5] * 1.01
    return o.to(BF16).view(B, Hq * D)


# ----------------------------------------------------------------------------------------------------------------- needles
def needle_positions(D):
    """The chunk and round edges, and a diagonal i -> chunk i, slot i % NT, key group i % KG (16 keys: every key group, slot and wave, two trips)."""
    KG, NT, CK, ROUND = geometry(D)
    L = longest(D)
    edges = {0, KG - 1, KG, CK - 1, CK, 3 * CK - 1, 3 * CK, ROUND - 1, ROUND, ROUND + CK, L - 1}
    diagonal = {i * CK + (i % NT) * KG + i % KG for i in range(16)}
    assert max(diagonal) < L
    return sorted(edges | diagonal)


@lru_cache(maxsize=None)
def build_needles(D):
    """Hq = Hkv = 2, one sample per needle position -> the namespace of ``build`` plus pos (list) and want bf16 [B, 2 D] = v[b, pos[b]]."""
    pos = needle_positions(D)
    B, H, L = len(pos), 2, longest(D)
    cap = L + MARGIN
    g = torch.Generator().manual_seed(77 + D)
    q = torch.randn(B, H, D, generator=g)
    q = (q * (D ** 0.5 / q.norm(dim=-1, keepdim=True))).view(B, H * D).to(BF16)  # |q|^2 = D per head: the needle scores 8 sqrt(D) in every sample
    k = torch.randn(B, L, H * D, generator=g).to(BF16)
    v = torch.randn(B, L, H * D, generator=g).to(BF16)
    for b, j in enumerate(pos):
        k[b, j] = (8.0 * q[b].float()).to(BF16)
    ks, vs, ld = _caches(B, cap, H * D)
    cache_view(ks, B, cap, H * D, ld)[:, :L] = k
    cache_view(vs, B, cap, H * D, ld)[:, :L] = v
    want = torch.stack([v[b, j] for b, j in enumerate(pos)])
    return SimpleNamespace(q=q, ks=ks, vs=vs, ld=ld, cap=cap, km_wide=None, vis=torch.ones(B, L, dtype=torch.bool), L=L, host_len=L, len_dev=None,
                           scale=D ** -0.5, B=B, Hq=H, Hkv=H, D=D, pos=pos, want=want)


# ----------------------------------------------------------------------------------------------------------------- gemv
GEMV_SHAPES = ((1, 8), (3, 504), (5, 512), (1001, 520), (4099, 1032), (2, 3072))  # (N, K)
GEMV_PRO_SHAPES = ((3, 40, 3072), (8, 20, 1032), (5, 8201, 520), (1, 3, 8))  # (M, N, K)


def nan_framed(t, left, right):
    """[rows, left + cols + right] of NaN with t in the middle -> (the wide tensor, the view onto t's columns)"""
    wide = torch.full((t.shape[0], left + t.shape[1] + right), float("nan"), dtype=t.dtype)
    wide[:, left : left + t.shape[1]] = t
    return wide, wide[:, left : left + t.shape[1]]


@lru_cache(maxsize=None)
def gemv_case(N, K):
    """Operands for M = 8 rows (M < 8 uses the first M) -> namespace(x [8, K], w [N, K], r [8, N] bf16, dense)"""
    g = torch.Generator().manual_seed(13 * N + K)
    x = torch.randn(8, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    r = torch.randn(8, N, generator=g).to(BF16)
    return SimpleNamespace(x=x, w=w, r=r)


def gemv_exact(ns, M, residual):
    """-> namespace(ref fp64 [M, N], weight = sum_k |x| |w| + |r|, c_raw, c)"""
    x, w, r = ns.x[:M], ns.w, ns.r[:M]
    ref = x.double() @ w.double().T
    ref32 = x.float() @ w.float().T
    weight = x.double().abs() @ w.double().abs().T
    if residual:
        ref, ref32, weight = ref + r.double(), ref32 + r.float(), weight + r.double().abs()
    raw, c = measure_c(ref32, ref, weight)
    return SimpleNamespace(ref=ref, weight=weight, c_raw=raw, c=c)


def judge_gemv(y, ex, label):
    """Element by element: |y - ref64| <= 2^-7 |ref64| + c (sum |x| |w| + |r|); -> failure strings naming row and column"""
    y = y.detach().cpu().double()
    if not bool(torch.isfinite(y).all()):
        m, n = (~torch.isfinite(y)).nonzero()[0].tolist()
        return [f"{label}: not finite at row {m}, column {n}"]
    over = (y - ex.ref).abs() - (OUT_ROUNDING * ex.ref.abs() + ex.c * ex.weight)
    if bool((over > 0).any()):
        m, n = divmod(int(over.argmax()), y.shape[1])
        return [f"{label}: row {m}, column {n}: |{float(y[m, n]):.6e} - {float(ex.ref[m, n]):.6e}| exceeds the bound by {float(over[m, n]):.3e} "
                f"(c = {ex.c:.2e}; {int((over > 0).sum())} elements)"]
    return []


# ----------------------------------------------------------------------------------------------------------------- argmax
ARG_SPLIT = 64
ARGMAX_V = (1, 63, 64, 65, 257, 16385)
IN_RANGE = -1  # expected value of a row that holds NaN: any index of the row


def first_maximum(row):
    """Plain Python: first index of the row maximum"""
    vals = row.float().tolist()
    best, idx = vals[0], 0
    for i, x in enumerate(vals):
        if x > best:
            best, idx = x, i
    return idx


@lru_cache(maxsize=None)
def argmax_case(V):
    """-> (x bf16 [P, V], want: list of P expected indices (IN_RANGE for rows with NaN), names: list of P pattern names, first: the row of the first
    pattern of each kind)."""
    g = torch.Generator().manual_seed(V)
    span = (V + ARG_SPLIT - 1) // ARG_SPLIT
    rows, names = [], []

    def base():
        return torch.randn(V, generator=g).clamp_(-4, 4)

    def add(name, row):
        rows.append(row)
        names.append(name)

    planted = {0, V - 1} | {i for k in range(1, ARG_SPLIT + 1) for i in (k * span - 1, k * span) if 0 <= i < V}
    for i in sorted(planted):
        r = base()
        r[i] = 9.0
        add("max at a range edge", r)
    ties = [(span - 1, span), (span - 1, V - 1), (0, V - 1)]  # across the first range boundary, across many ranges, end to end
    if span > 64:
        ties += [(span + 63, span + 64), (span + 63, span + 128)]  # across a wave boundary inside range 1
    if span > 256:
        ties += [(span + 255, span + 256)]  # a thread's first and second column
    for a, b in ties:
        if 0 <= a < b < V:
            r = base()
            r[a] = r[b] = 9.0
            add("tie across a boundary", r)
    add("all equal", torch.full((V,), 1.5))
    add("all negative", -base().abs() - 0.5)
    for i in sorted({V // 2, V - 1}):
        r = torch.full((V,), -math.inf)
        r[i] = -3.0
        add("one finite entry among -inf", r)
    add("all -inf", torch.full((V,), -math.inf))
    add("all NaN", torch.full((V,), math.nan))
    r = base()
    r[V // 3] = math.nan
    add("one NaN", r)
    r = torch.full((V,), -math.inf)
    r[V - 1] = math.nan
    add("NaN among -inf", r)
    x = torch.stack(rows).to(BF16)
    want = [IN_RANGE if bool(torch.isnan(r).any()) else first_maximum(r) for r in x]
    first = [names.index(n) for n in dict.fromkeys(names)]
    return x, want, names, first
