"""The fp64 sweep of the row kernels -- csrc/norm_rope.hip (RMSNorm, QK-norm + RoPE, LayerNorm, reduce_rows) and the SwiGLU / GELU kernels of
csrc/elementwise.hip: case tables, operand builders, fp64 references, an fp32 emulation per kernel family and the judgement shared by
test_row_sweep_cpu.py and test_row_sweep_gpu.py.  TEST INFRASTRUCTURE ONLY.

Geometry.  Every row kernel is "one wave per row (token), four waves per block, a capped grid, then a grid-stride loop"; the element kernels are "one
16-byte vector per thread, 256 threads per block, 2048 blocks, then a grid-stride loop".  ``GEOMETRY`` states the caps, the vector widths, the widths
that dispatch to a row-in-registers kernel, the stated maxima and the heads per pass ONCE; every case and every coverage claim (``trips``,
``last_trip_partial``, ``lane_vectors``, ``branch``, ``head_passes``, ``element_trips``) is derived from it.

Operands.  Every floating-point input is a contiguous slice, at a 16-byte-aligned offset, of a larger 1-D storage whose other elements are NaN
(``framed``).  Caller-provided outputs are pre-filled with the bit pattern 0x5A5A(5A5A) (``filled``); a destination that is accumulated into holds
random data.  Per case one row is all zero (a padding row), one is scaled by 2^6 and one by 2^-6 (``special_rows``: all three from 3 rows on, the 2^6 row
alone below; LayerNorm gets no zero row, both modes are singular on a constant row).  No pointer is misaligned, no position leaves the RoPE table.

Judgement (``judge``), per unit (row; token and head for QK-norm + RoPE; column for the parameter gradients; 16-byte vector for GELU), element by element:
    |got - ref64| <= R * 2^-7 * |term| + c * magnitude (+ underflow, SwiGLU / GELU only).
R counts the bf16 roundings the kernel's comments document on the way to the element (0 for fp32 outputs; 1 for RMSNorm, LayerNorm, GELU and every
gradient that is stored as bf16; 2 for the SwiGLU forward; 3 for the QK-norm + RoPE forward, where ``term`` is |c n1| + |s n2|, the magnitude the
roundings act on; the lo half of a split3 output is one rounding of a value below 2^-8 |y|: 2^-15 |ref|).  2^-7 is twice the half-ulp of bf16, because the
rounded value is itself an fp32 result.  ``magnitude`` is the sum of the absolute values of the terms the formula adds for the element.  c covers the fp32
arithmetic and is MEASURED per case (``measure_c``): the largest |ref32 - ref64| / magnitude of a plain fp32 torch evaluation of the same formula, times
64 (another summation order, hardware rsqrt / rcp / exp), floor 2^-20, cap 2^-10 -- the figures of decode_sweep.py, kept.  The cap is a condition on the
inputs: the CPU test asserts it for every case.
Underflow term (the one departure from the plain form, SwiGLU and GELU only).  The special values +-88, +-89, +-100, +-1000 drive sigmoid(g) and
the products built on it below 2^-126, the smallest normal number of fp32 AND of bf16.  There no arithmetic is relatively accurate: fp32 torch itself
returns sigmoid(-89) = 0 where fp64 has 2.2e-39, and silu(-100) u = 3.7e-42 u is not a bf16 number at all.  An intermediate lost below 2^-126 is wrong by
at most 2^-126 absolutely, and reaches the output times the factors that multiply it afterwards; so these two families add 2^-126 * max(1, that
factor) (|g u| for the SwiGLU forward, |d g| and |d u| (1 + |g|) for its gradients, |x| and |dy| max(1, |x|) for GELU) to the bound and subtract it in
``measure_c``.  It is below 1e-33 in every case and changes nothing for an element in the normal range.
A NaN or Inf in an output fails the case and names the unit.  No unit is left out: ``judge`` returns how many it judged and the tests assert that count
against ``units`` (computed from the case alone).

Tighter criterion for the forwards whose rounding points the emulation reproduces exactly (RMSNorm, QK-norm + RoPE, SwiGLU; ``steps_from``): at most one
bf16 step from the emulation on at most 2e-3 of the elements (never less than one element: a share cannot be finer than 1 / numel).  Taken literally
against a free-standing emulation this is unsound for an output behind MORE than one rounding, and the first GPU run showed it (QK forward, 8195
tokens: one element of 1,048,960 four steps away; SwiGLU 1366 x 3080: one element of 4,207,280 two steps away; every fp64 bound held): when the fp32
value in front of an INNER rounding point differs in its last bit (another summation order under rstd; a hardware exp and reciprocal under sigmoid),
that rounding now and then falls to the neighbouring bf16 value, the product built on it moves by up to two of its own steps, and a sum of two such
products that cancel by more steps still.  So the comparison is made where it is sound, without widening the step:
  * RMSNorm and QK-norm + RoPE: the emulation takes the kernel's own rstd (an output, judged against fp64 on its own).  Everything behind it is
    single IEEE multiplications, additions and roundings in the documented order, so the comparison is one step at most at every rounding point -- and
    in fact bit for bit.
  * SwiGLU: the hardware sigmoid cannot be handed over, so the one-step allowance is applied at each rounding point: the inner bf16 tensor silu(g) may be
    the emulated value or its neighbour on either side, and the output must be within one step of the product built on one of the three; the share
    counts every element that differs from the plain emulation.  Elements whose emulated value is below 2^-100 in magnitude are left to the fp64 bound
    (the hardware exp / rcp flush where the CPU keeps subnormals, see above).  test_row_sweep_cpu.py shows both halves: an emulation whose sigmoid is
    off by one part in 2^23 passes this form.

Measured (``MEASURED`` below holds the same figures).  c per family over all its cases, on an x86-64 host with torch's fp32 CPU kernels (the figure
depends on the host's summation order; test_row_sweep_cpu.py prints it again on every run), and the largest error / bound seen on an MI355X:
    family        geometry                                                      rule (R)                       c                       GPU error / bound
    rmsnorm       wave per row, 2048 / 512 blocks, rowreg 1024 | 512, 1024      y, dx, bf16 dw 1; rstd, dw 0   4.6e-6 .. 1.7e-5        0.497
    reduce_rows   16 part-lanes x 4-way unroll, 64 columns per block            bf16 1, fp32 0                 floor 9.5e-7 .. 1.9e-5  0.496
    qknorm_rope   wave per token, HPW 16 | 8 heads per pass, 2048 / 768 blocks  y 3 (on |c n1| + |s n2|), d 1  floor .. 1.9e-5         0.498
    layernorm     wave per row, 2048 / 1024 blocks, rowreg 768, 1024            bf16 1, split3 2^-8, fp32 0    1.9e-6 .. 1.5e-5        0.497 (fp32 outputs: 0.02)
    swiglu_gelu   vector per thread, 2048 x 256 threads per trip                a 2; du, dg, y, dx 1           floor .. 6.3e-5         0.844 (SwiGLU), 0.497 (GELU)
The cap is 9.8e-4.  With c this small the bound of a bf16 output is its rounding term almost everywhere: emulation and kernels both use half of it.  The
three launches at a stated maximum (forward width 8192; backward width 4096 and LayerNorm backward width 2048, 65,536 bytes of dynamic LDS each) run and
are judged like every other case: the runtime accepts them, so the stated limits are true as they stand.
"""

from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
C_FLOOR, C_CAP, C_FACTOR = 2.0 ** -20, 2.0 ** -10, 64.0  # decode_sweep.py's figures, kept
ROUNDING = 2.0 ** -7
SPLIT3_LO = 2.0 ** -8  # R of a split3 output: one rounding of the lo half, which is below 2^-8 |y|
TINY = 2.0 ** -126  # smallest normal number of fp32 and of bf16
STEP_SHARE = 2e-3  # what assert_bf16_within_1ulp allows
STEP_FLOOR = 2.0 ** -100

# ----------------------------------------------------------------------------------------------------------------- geometry
# csrc/norm_rope.hip, csrc/elementwise.hip and the wrappers of llm_quest_amd/kernels.py.  cap: most blocks of a launch; vec: elements per 16-byte vector;
# rowreg: widths that take a row-in-registers kernel (value: vectors per lane); max_width: the entry's stated maximum; HPW: heads per wave and pass.
ROWS_PER_BLOCK, LANES = 4, 64
NORM_PARTS, QK_PARTS, LN_BWD_PARTS = 512, 768, 1024
GEOMETRY = {
    "rmsnorm_fwd": dict(cap=2048, vec=8, rowreg={1024: 2}, max_width=8192),
    "rmsnorm_bwd": dict(cap=NORM_PARTS, vec=8, rowreg={512: 1, 1024: 2}, max_width=4096, lds_bytes_per_col=16),
    "qk_fwd": dict(cap=2048, vec=8, HPW={64: 16, 128: 8}),
    "qk_bwd": dict(cap=QK_PARTS, vec=8, HPW={64: 16, 128: 8}, wrapper_hpw={64: 8, 128: 4}),  # wrapper_hpw: what kernels.qknorm_rope_bwd sizes the grid by
    "layernorm_fwd": dict(cap=2048, vec=4, rowreg={768: 3, 1024: 4}, max_width=None),
    "layernorm_bwd": dict(cap=LN_BWD_PARTS, vec=4, rowreg={768: 3, 1024: 4}, max_width=2048, lds_bytes_per_col=32),
    "reduce_rows": dict(part_lanes=16, unroll=4, cols_per_block=64),
    "swiglu": dict(cap=2048, threads=256, vec=8),
    "gelu": dict(cap=2048, threads=256, vec=8),
}


def blocks(kernel, rows, cap=None):
    cap = GEOMETRY[kernel]["cap"] if cap is None else cap
    return max(1, min(cap, (rows + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK))


def trips(kernel, rows, cap=None):
    """trips of the busiest wave (wave 0 of block 0) through the row loop"""
    return -(-rows // (ROWS_PER_BLOCK * blocks(kernel, rows, cap)))


def last_trip_partial(kernel, rows, cap=None):
    """more than one trip, and the last one does not reach every wave"""
    return trips(kernel, rows, cap) > 1 and rows % (ROWS_PER_BLOCK * blocks(kernel, rows, cap)) != 0


def first_wrap(kernel):
    """cap blocks of four rows, plus three: three waves of block 0 take a second row, the fourth does not"""
    return GEOMETRY[kernel]["cap"] * ROWS_PER_BLOCK + 3


def lane_vectors(kernel, width):
    """vectors the busiest lane handles per sweep over a row"""
    return -(-(width // GEOMETRY[kernel]["vec"]) // LANES)


def branch(kernel, width):
    return f"rowreg{GEOMETRY[kernel]['rowreg'][width]}" if width in GEOMETRY[kernel]["rowreg"] else "generic"


def element_trips(kernel, vectors):
    g = GEOMETRY[kernel]
    per_trip = g["threads"] * min(g["cap"], max(1, -(-vectors // g["threads"])))
    return -(-vectors // per_trip)


def head_passes(D, Hq, Hkv, konly=False):
    """-> the passes of one token: each a tuple of HPW slots holding 'q', 'k' or None (an idle slot)"""
    hpw = GEOMETRY["qk_fwd"]["HPW"][D]
    heads = ([] if konly else ["q"] * Hq) + ["k"] * Hkv
    out = []
    for p in range(-(-len(heads) // hpw)):
        s = heads[p * hpw : (p + 1) * hpw]
        out.append(tuple(s + [None] * (hpw - len(s))))
    return out


def reduce_walk(parts, lane):
    """-> (trips of part-lane ``lane`` through reduce_rows_kernel's unrolled loop, steps of its tail)"""
    g = GEOMETRY["reduce_rows"]
    step, reach = g["part_lanes"] * g["unroll"], g["part_lanes"] * (g["unroll"] - 1)
    p, unrolled, tail = lane, 0, 0
    while p + reach < parts:
        p, unrolled = p + step, unrolled + 1
    while p < parts:
        p, tail = p + g["part_lanes"], tail + 1
    return unrolled, tail


def qk_parts(tokens, Hq, Hkv, D, cap=None):
    cap = QK_PARTS if cap is None else cap
    hpw = GEOMETRY["qk_bwd"]["wrapper_hpw"][D]
    return min(cap, (tokens * ((Hq + Hkv + hpw - 1) // hpw) + 3) // 4)


# ----------------------------------------------------------------------------------------------------------------- operands
PAD = 64  # elements in front of and behind a framed operand: 128 or 256 bytes


def framed(t, device="cpu"):
    """t as a contiguous slice, at a 16-byte-aligned offset, of a 1-D storage of NaN"""
    if t is None:
        return None
    if not t.is_floating_point():
        return t.to(device)
    flat = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype)
    flat[PAD : PAD + t.numel()] = t.reshape(-1)
    flat = flat.to(device)
    v = flat[PAD : PAD + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


def filled(shape, dtype, device="cpu"):
    """a caller-provided destination, pre-filled with a fixed non-zero bit pattern"""
    if dtype == BF16:
        return torch.full(tuple(shape), 0x5A5A, dtype=torch.int16, device=device).view(BF16)
    assert dtype == F32
    return torch.full(tuple(shape), 0x5A5A5A5A, dtype=torch.int32, device=device).view(F32)


def holds_fill(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == BF16:
        return bool((t.view(torch.int16) == 0x5A5A).all())
    return bool((t.view(torch.int32) == 0x5A5A5A5A).all())


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def special_rows(x, zero=True):
    """in place: row 0 times 2^6; from three rows on, row 1 all zero (if ``zero``) and the last row times 2^-6"""
    x[0] *= 64.0
    if x.shape[0] >= 3:
        if zero:
            x[1] = 0.0
        x[-1] *= 2.0 ** -6
    return x


def rbf(t):
    """round through bf16, stay fp32"""
    return t.to(BF16).to(F32)


def seed_of(case):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(case.name)) % (2 ** 31)


# ----------------------------------------------------------------------------------------------------------------- the judgement
Out = namedtuple("Out", "ref term mag R unit tiny")  # ref, term, mag: [units, elements]; R: roundings (float); unit: what a row of ref is called


def out(ref, mag, R, unit, term=None, tiny=0.0):
    ref = ref if ref.dim() == 2 else ref.reshape(ref.shape[0], -1)
    shape = ref.shape
    fix = lambda t: t.reshape(shape) if torch.is_tensor(t) else t
    return Out(ref, ref if term is None else fix(term), fix(mag), float(R), unit, fix(tiny))


def col(v):
    return v.reshape(-1, 1)


def measure_c(outs32, outs64):
    """-> (64 x the fp32 evaluation's largest error per unit of magnitude, the c of the bound: that figure under the floor)"""
    raw = 0.0
    for name, o in outs64.items():
        err = ((outs32[name].ref.double() - o.ref).abs() - o.tiny).clamp_min(0.0)
        ratio = torch.where(err > 0, err / o.mag.clamp_min(1e-300), torch.zeros_like(err))
        raw = max(raw, float(ratio.max()))
    raw *= C_FACTOR
    return raw, max(raw, C_FLOOR)


def judge(got, ex, label):
    """got: name -> tensor, one per output of ``ex.outs`` -> (units judged, failure strings naming output, unit and element, largest error / bound)"""
    judged, fails, worst = 0, [], 0.0
    for name, o in ex.outs.items():
        g = got[name].detach().cpu().double().reshape(o.ref.shape)
        judged += g.shape[0]
        fin = torch.isfinite(g)
        bound = o.R * ROUNDING * o.term.abs() + ex.c * o.mag + o.tiny
        err = torch.where(fin, (g - o.ref).abs(), torch.zeros_like(g))
        ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        worst = max(worst, float(ratio.max()))
        over = err > bound
        for u in ((~fin).any(1) | over.any(1)).nonzero().flatten().tolist()[:3]:
            if not bool(fin[u].all()):
                fails.append(f"{label}: {name}, {o.unit} {u}: not finite at element {int((~fin[u]).nonzero()[0])}")
            else:
                e = int((err[u] - bound[u]).argmax())
                fails.append(f"{label}: {name}, {o.unit} {u}, element {e}: |{float(g[u, e]):.6e} - {float(o.ref[u, e]):.6e}| > {float(bound[u, e]):.3e} "
                             f"(c = {ex.c:.2e}; {int(over[u].sum())} of {g.shape[1]} elements)")
    return judged, fails, worst


def units(ex):
    return sum(o.ref.shape[0] for o in ex.outs.values())


def finish(outs64, outs32):
    raw, c = measure_c(outs32, outs64)
    return SimpleNamespace(outs=outs64, c_raw=raw, c=c)


def report(family, label, ex, worst=None):
    print(f"[row sweep] {family} {label}: c = {ex.c:.3e} (64 x fp32 reference error {ex.c_raw:.3e})" + ("" if worst is None else f", largest error / bound {worst:.3f}"))


def ordered(t):
    i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def bf16_step(t, k):
    """bf16 -> the value k steps further from zero (k = 1) or nearer to it (k = -1, zero stays zero)"""
    i = t.detach().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = ((i & 0x7FFF) + k).clamp_(0, 0x7F7F)
    j = (i & 0x8000) | mag
    return torch.where(j >= 0x8000, j - 0x10000, j).to(torch.int16).view(BF16)


def steps_from(got, emu, label, floor=None, alternatives=()):
    """the tighter criterion -> failure strings: bf16 ``got`` is at most one step from ``emu`` on at most STEP_SHARE of the elements.  ``alternatives``:
    further emulations (an inner rounding point one step up or down); the distance is then to the nearest of them, the share still counts every
    element that differs from ``emu`` itself."""
    got, emu = got.detach().cpu().reshape(-1), emu.detach().cpu().reshape(-1)
    assert got.dtype == BF16 and emu.dtype == BF16 and got.shape == emu.shape
    first = (ordered(got) - ordered(emu)).abs()
    d = first
    for alt in alternatives:
        d = torch.minimum(d, (ordered(got) - ordered(alt.detach().cpu().reshape(-1))).abs())
    if floor is not None:
        keep = emu.float().abs() >= floor
        d, first = d[keep], first[keep]
    if d.numel() == 0:
        return []
    fails = []
    if int(d.max()) > 1:
        fails.append(f"{label}: {int(d.max())} bf16 steps from the emulation at element {int(d.argmax())}")
    allowed = max(1, int(STEP_SHARE * d.numel()))
    if int((first != 0).sum()) > allowed:
        fails.append(f"{label}: {int((first != 0).sum())} of {d.numel()} elements differ from the emulation (allowed {allowed})")
    return fails


# ----------------------------------------------------------------------------------------------------------------- shared emulation pieces
def partition_sum(contrib, parts, drop_last_trip=False):
    """contrib fp32 [rows, n] -> partial [parts, n] as the backward kernels form it: a wave adds its rows in trip order, the block adds its four waves
    ((w0 + w1) + w2) + w3.  drop_last_trip (a planted defect): wave 0 of block 0 leaves out its last trip."""
    rows, n = contrib.shape
    per = parts * ROWS_PER_BLOCK
    t = -(-rows // per)
    c = torch.zeros(t * per, n, dtype=F32)
    c[:rows] = contrib
    c = c.view(t, parts, ROWS_PER_BLOCK, n)
    if drop_last_trip:
        assert t > 1
        c = c.clone()
        c[t - 1, 0, 0] = 0.0
    acc = torch.zeros(parts, ROWS_PER_BLOCK, n, dtype=F32)
    for i in range(t):
        acc = acc + c[i]
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]


def reduce_rows_emulated(partial, out_dtype=F32, old=None, drop_tail=False):
    """reduce_rows_kernel's order: part p goes to part-lane p % 16; a lane walks p, p + 16, p + 32, p + 48 into four sums while p + 48 < parts, then a
    tail into the first sum; (s0 + s1) + (s2 + s3); the sixteen lanes in order; (+ old); one rounding if the output is bf16."""
    parts, n = partial.shape
    red = []
    for rl in range(16):
        s = [torch.zeros(n, dtype=F32) for _ in range(4)]
        p = rl
        while p + 48 < parts:
            for k in range(4):
                s[k] = s[k] + partial[p + 16 * k]
            p += 64
        while p < parts and not drop_tail:
            s[0] = s[0] + partial[p]
            p += 16
        red.append((s[0] + s[1]) + (s[2] + s[3]))
    tot = torch.zeros(n, dtype=F32)
    for r in red:
        tot = tot + r
    if old is not None:
        tot = tot + old.float()
    return tot.to(out_dtype)


# ================================================================================================================= RMSNorm
RMS_EPS = 1e-6
RMS_FWD_WIDTHS = (8, 64, 504, 512, 520, 1016, 1024, 1032, 2048, 4096, 8192)
RMS_BWD_WIDTHS = (8, 64, 504, 512, 520, 1016, 1024, 1032, 4096)
SMALL_ROWS = (1, 3, 4, 5)
RmsCase = namedtuple("RmsCase", "name kind rows width want_rstd dres parts dw_dtype dw_acc hot")
RMS_DEFECTS = ("mean_over_padded_vectors", "drop_last_trip")


def _rms(kind, rows, width, want_rstd=True, dres=False, parts=None, dw_dtype=None, dw_acc=False, hot=None, tag=""):
    name = f"rms-{kind}-{rows}x{width}" + ("-nostat" if not want_rstd else "") + ("-dres" if dres else "") + (f"-parts{parts}" if parts else "") + \
        (f"-dw{'bf16' if dw_dtype == BF16 else 'f32'}{'+' if dw_acc else ''}" if dw_dtype is not None else "") + (f"-hot{hot}" if hot is not None else "") + tag
    return RmsCase(name, kind, rows, width, want_rstd, dres, parts, dw_dtype, dw_acc, hot)


def rms_fwd_cases():
    out = [_rms("fwd", SMALL_ROWS[i % 4], w) for i, w in enumerate(RMS_FWD_WIDTHS)]
    out += [_rms("fwd", first_wrap("rmsnorm_fwd"), w) for w in (8, 520, 1024)]
    out += [_rms("fwd", 5, w, want_rstd=False) for w in (64, 1024)]  # one per kernel
    return out


RMS_WRAP_BWD = 4 * NORM_PARTS + 5  # 2053 rows: five waves take a second row under the default parts


def rms_bwd_cases():
    out = []
    for i, w in enumerate(RMS_BWD_WIDTHS):
        out += [_rms("bwd", SMALL_ROWS[i % 4], w), _rms("bwd", SMALL_ROWS[(i + 1) % 4], w, dres=True), _rms("bwd", 50, w, dres=i % 2 == 0, parts=3)]
    out += [_rms("bwd", RMS_WRAP_BWD, w, dres=True) for w in (512, 520, 1024)]
    for w in (512, 520, 1024):  # one width per kernel
        out += [_rms("bwd", 5, w, dw_dtype=dt, dw_acc=acc) for dt in (BF16, F32) for acc in (False, True)]
    return out


def rms_structural_cases():
    """more rows than one grid trip, the upstream gradient zero except in one row"""
    return [_rms("bwd", RMS_WRAP_BWD, w, dres=dres, hot=2050) for w, dres in ((512, True), (520, False), (1024, True))]


@lru_cache(maxsize=4)
def rms_build(case):
    g = torch.Generator().manual_seed(seed_of(case))
    rows, width = case.rows, case.width
    x = special_rows(torch.randn(rows, width, generator=g) * 2).to(BF16)
    w = (1 + 0.1 * torch.randn(width, generator=g)).to(BF16)
    ns = SimpleNamespace(x=x, w=w, dy=None, dres=None, old=None)
    if case.kind == "bwd":
        dy = torch.randn(rows, width, generator=g)
        if case.hot is not None:
            keep = dy[case.hot].clone()
            dy.zero_()
            dy[case.hot] = keep
        ns.dy = dy.to(BF16)
        ns.dres = torch.randn(rows, width, generator=g).to(BF16) if case.dres else None
        if case.dw_dtype is not None and case.dw_acc:
            ns.old = (3 * torch.randn(width, generator=g)).to(case.dw_dtype)
    return ns


def rms_parts(case):
    return min(case.parts or NORM_PARTS, (case.rows + 3) // 4)


def rms_reference(case, ns, dt):
    x, w = ns.x.to(dt), ns.w.to(dt)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + RMS_EPS)
    if case.kind == "fwd":
        y = x * r * w
        outs = {"y": out(y, y.abs(), 1, "row")}
        if case.want_rstd:
            outs["rstd"] = out(r, r.abs(), 0, "row")
        return outs
    dy = ns.dy.to(dt)
    xhat, gw = x * r, w * dy
    dx = r * (gw - xhat * (gw * xhat).mean(-1, keepdim=True))
    mag = r * (gw.abs() + xhat.abs() * (gw * xhat).abs().mean(-1, keepdim=True))
    if ns.dres is not None:
        dx, mag = dx + ns.dres.to(dt), mag + ns.dres.to(dt).abs()
    dw, dwm = (dy * xhat).sum(0), (dy * xhat).abs().sum(0)
    if ns.old is not None:
        dw, dwm = dw + ns.old.to(dt), dwm + ns.old.to(dt).abs()
    return {"dx": out(dx, mag, 1, "row"), "dw": out(col(dw), col(dwm), 1 if case.dw_dtype == BF16 else 0, "column")}


@lru_cache(maxsize=4)
def rms_exact(case):
    ns = rms_build(case)
    return finish(rms_reference(case, ns, F64), rms_reference(case, ns, F32))


def rms_emulate(case, defect=None, rstd=None):
    """fp32, the products in the kernels' order, one bf16 rounding per output; dw per wave, per block, over the parts.  ``rstd`` (fp32 [rows]): the
    kernel's own, in place of the emulated one -- the products that follow are then the kernel's bit for bit.  Defects --
    mean_over_padded_vectors: the mean of squares is divided by the padded vector count times 8, not by the width; drop_last_trip: see partition_sum."""
    assert defect is None or defect in RMS_DEFECTS
    ns = rms_build(case)
    x, w, width = ns.x.float(), ns.w.float(), case.width
    denom = float(lane_vectors("rmsnorm_fwd", width) * LANES * 8) if defect == "mean_over_padded_vectors" else float(width)
    r = torch.rsqrt((x * x).sum(-1, keepdim=True) / denom + RMS_EPS) if rstd is None else rstd.detach().cpu().float().reshape(-1, 1)
    if case.kind == "fwd":
        got = {"y": (x * r * w).to(BF16)}
        if case.want_rstd:
            got["rstd"] = r
        return got
    dy = ns.dy.float()
    dot = ((dy * w) * x).sum(-1, keepdim=True) * r * r / float(width)
    dx = r * (dy * w - x * dot)
    if ns.dres is not None:
        dx = dx + ns.dres.float()
    partial = partition_sum(dy * x * r, rms_parts(case), drop_last_trip=defect == "drop_last_trip")
    return {"dx": dx.to(BF16), "dw": reduce_rows_emulated(partial, case.dw_dtype or F32, ns.old)}


# ================================================================================================================= reduce_rows
RED_PARTS = (1, 15, 16, 17, 48, 49, 64, 65, 113, 512)
RED_N = (1, 63, 64, 65, 256, 1032)
RedCase = namedtuple("RedCase", "name parts n dtype acc")
RED_DEFECTS = ("drop_tail",)


def red_cases():
    """every part count with every output form; the column counts rotate"""
    out = []
    for i, p in enumerate(RED_PARTS):
        for j, (dt, acc) in enumerate(((F32, 0), (F32, 1), (BF16, 0), (BF16, 1))):
            n = RED_N[(i + j) % len(RED_N)]
            out.append(RedCase(f"reduce-p{p}-n{n}-{'bf16' if dt == BF16 else 'f32'}{'+' if acc else ''}", p, n, dt, acc))
    return out


@lru_cache(maxsize=None)
def red_build(case):
    g = torch.Generator().manual_seed(seed_of(case))
    part = special_rows(torch.randn(case.parts, case.n, generator=g))
    old = (3 * torch.randn(case.n, generator=g)).to(case.dtype) if case.acc else None
    return SimpleNamespace(part=part, old=old)


def red_reference(case, ns, dt):
    s, m = ns.part.to(dt).sum(0), ns.part.to(dt).abs().sum(0)
    if ns.old is not None:
        s, m = s + ns.old.to(dt), m + ns.old.to(dt).abs()
    return {"out": out(col(s), col(m), 1 if case.dtype == BF16 else 0, "column")}


@lru_cache(maxsize=None)
def red_exact(case):
    ns = red_build(case)
    return finish(red_reference(case, ns, F64), red_reference(case, ns, F32))


def red_emulate(case, defect=None):
    assert defect is None or defect in RED_DEFECTS
    ns = red_build(case)
    return {"out": reduce_rows_emulated(ns.part, case.dtype, ns.old, drop_tail=defect == "drop_tail")}


# ================================================================================================================= QK-norm + RoPE
QK_EPS = 1e-6
QK_HEADS = ((1, 1), (4, 2), (7, 1), (7, 2), (16, 8), (16, 1), (9, 9), (17, 17), (8, 8))  # (8, 8): the one full single pass at D = 64
QK_FORMS = ("fwd", "fwd_rope", "bwd", "bwd_k", "bwd_rope")
QK_TOKENS = (1, 3, 5)
QK_CTX = 40  # rows of the rotary table
QkCase = namedtuple("QkCase", "name form D Hq Hkv tokens parts hot")
QK_DEFECTS = ("key_heads_with_query_weight", "second_pass_unwritten")
QK_WRAP_BWD = 4 * QK_PARTS + 5  # 3077 tokens


def _qk(form, D, Hq, Hkv, tokens, parts=None, hot=None):
    return QkCase(f"qk-{form}-D{D}-H{Hq}x{Hkv}-T{tokens}" + (f"-parts{parts}" if parts else "") + (f"-hot{hot}" if hot is not None else ""), form, D, Hq, Hkv, tokens, parts, hot)


def qk_cases():
    out = []
    for di, D in enumerate((64, 128)):
        for hi, (Hq, Hkv) in enumerate(QK_HEADS):
            for fi, form in enumerate(QK_FORMS):
                out.append(_qk(form, D, Hq, Hkv, QK_TOKENS[(di + hi + fi) % 3]))
    out.append(_qk("fwd", 64, 1, 1, first_wrap("qk_fwd")))
    for D in (64, 128):
        for form in ("bwd", "bwd_k"):
            out += [_qk(form, D, 4, 2, 21, parts=2), _qk(form, D, 9, 9, 21, parts=2)]
        out += [_qk("bwd", D, 4, 2, QK_WRAP_BWD), _qk("bwd_k", D, 4, 2, QK_WRAP_BWD)]
    return out


def qk_structural_cases():
    return [_qk(form, D, 4, 2, QK_WRAP_BWD, hot=3075) for D in (64, 128) for form in ("bwd", "bwd_k")]  # the key-only form is a kernel of its own


def qk_positions(tokens):
    """non-monotonic, with repeats, the table's last row and row 0 as far as the tokens reach; never outside the table"""
    pos = [(7 * t + 3) % QK_CTX for t in range(tokens)]
    pos[0] = QK_CTX - 1
    if tokens >= 2:
        pos[1] = 0
    if tokens >= 3:
        pos[2] = QK_CTX - 1
    assert 0 <= min(pos) and max(pos) < QK_CTX
    return torch.tensor(pos, dtype=torch.int32)


@lru_cache(maxsize=4)
def qk_build(case):
    g = torch.Generator().manual_seed(seed_of(case))
    D, Hq, Hkv, T = case.D, case.Hq, case.Hkv, case.tokens
    qkv = special_rows(torch.randn(T, (Hq + 2 * Hkv) * D, generator=g)).to(BF16)
    norm = not case.form.endswith("rope")
    qw = (1 + 0.1 * torch.randn(D, generator=g)).to(BF16) if norm else None
    kw = (1 + 0.1 * torch.randn(D, generator=g)).to(BF16) if norm else None
    # a rotary table whose two halves differ (angle + 0.1 in the second): the kernels read c1, s1, c2, s2 from their own columns
    ang = torch.arange(QK_CTX, dtype=F32)[:, None] * torch.logspace(0, -3, D // 2)[None, :]
    cos, sin = torch.cat([ang.cos(), (ang + 0.1).cos()], 1).contiguous(), torch.cat([ang.sin(), (ang + 0.1).sin()], 1).contiguous()
    ns = SimpleNamespace(qkv=qkv, qw=qw, kw=kw, cos=cos, sin=sin, pos=qk_positions(T), dq=None, dk=None, norm=norm, konly=case.form == "bwd_k")
    if case.form.startswith("bwd"):
        dq, dk = torch.randn(T, Hq * D, generator=g), torch.randn(T, Hkv * D, generator=g)
        if case.hot is not None:
            for t in (dq, dk):
                keep = t[case.hot].clone()
                t.zero_()
                t[case.hot] = keep
        ns.dq, ns.dk = (None if ns.konly else dq.to(BF16)), dk.to(BF16)
    return ns


def _qk_heads(case, ns, dt):
    """-> x [T, H, D], w [H, D] (ones without norm), c, s [T, 1, D] from the bf16-rounded table, all in ``dt``"""
    D, Hq, Hkv, T = case.D, case.Hq, case.Hkv, case.tokens
    x = ns.qkv[:, : (Hq + Hkv) * D].to(dt).view(T, Hq + Hkv, D)
    if ns.norm:
        w = torch.cat([ns.qw.to(dt).expand(Hq, D), ns.kw.to(dt).expand(Hkv, D)], 0)
    else:
        w = torch.ones(Hq + Hkv, D, dtype=dt)
    p = ns.pos.long()
    return x, w, ns.cos[p].to(BF16).to(dt)[:, None, :], ns.sin[p].to(BF16).to(dt)[:, None, :]


def qk_reference(case, ns, dt):
    D, Hq, Hkv, T = case.D, case.Hq, case.Hkv, case.tokens
    H, h = Hq + Hkv, D // 2
    x, w, c, s = _qk_heads(case, ns, dt)
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + QK_EPS) if ns.norm else torch.ones(T, H, 1, dtype=dt)
    c1, c2, s1, s2 = c[..., :h], c[..., h:], s[..., :h], s[..., h:]
    if case.form.startswith("fwd"):
        n = x * r * w
        n1, n2 = n[..., :h], n[..., h:]
        y = torch.cat([c1 * n1 - s1 * n2, c2 * n2 + s2 * n1], -1)
        m = torch.cat([(c1 * n1).abs() + (s1 * n2).abs(), (c2 * n2).abs() + (s2 * n1).abs()], -1)
        outs = {"y": out(y.reshape(T * H, D), m, 3, "(token, head)", term=m)}
        if ns.norm:
            outs["rstd"] = out(r.reshape(T * H, 1), r.abs(), 0, "(token, head)")
        return outs
    h0 = Hq if ns.konly else 0
    gq = torch.zeros(T, Hq, D, dtype=dt) if ns.dq is None else ns.dq.to(dt).view(T, Hq, D)
    g = torch.cat([gq, ns.dk.to(dt).view(T, Hkv, D)], 1)
    g1, g2 = g[..., :h], g[..., h:]
    dn = torch.cat([c1 * g1 + s2 * g2, c2 * g2 - s1 * g1], -1)
    dnm = torch.cat([(c1 * g1).abs() + (s2 * g2).abs(), (c2 * g2).abs() + (s1 * g1).abs()], -1)
    if ns.norm:
        xh = x * r
        d = r * (dn * w - xh * (dn * w * xh).mean(-1, keepdim=True))
        dm = r * (dnm * w.abs() + xh.abs() * (dnm * w.abs() * xh.abs()).mean(-1, keepdim=True))
        dw, dwm = (dn * xh)[:, h0:], (dnm * xh.abs())[:, h0:]
    else:
        d, dm = dn, dnm
        dw, dwm = torch.zeros(T, H - h0, D, dtype=dt), torch.zeros(T, H - h0, D, dtype=dt)
    nq = Hq - h0
    return {"d": out(d[:, h0:].reshape(T * (H - h0), D), dm[:, h0:], 1, "(token, head)"),
            "dqw": out(col(dw[:, :nq].sum((0, 1))), col(dwm[:, :nq].sum((0, 1))), 0, "column"),
            "dkw": out(col(dw[:, nq:].sum((0, 1))), col(dwm[:, nq:].sum((0, 1))), 0, "column")}


@lru_cache(maxsize=4)
def qk_exact(case):
    ns = qk_build(case)
    return finish(qk_reference(case, ns, F64), qk_reference(case, ns, F32))


def qk_emulate(case, defect=None, rstd=None):
    """The documented rounding points of the forward: n = bf16(x r w), y1 = bf16(bf16(c1 n1) + bf16(s1 (-n2))), y2 = bf16(bf16(c2 n2) + bf16(s2 n1)); the
    backward in fp32 with one rounding; dw per (wave, head slot) over the wave's tokens and passes, the block's 4 HPW regions in order, reduce_rows.
    ``rstd`` (fp32 [tokens, heads]): the kernel's own in place of the emulated one.
    Defects -- key_heads_with_query_weight; second_pass_unwritten: the heads of the second pass keep the destination's fill."""
    assert defect is None or defect in QK_DEFECTS
    ns = qk_build(case)
    D, Hq, Hkv, T = case.D, case.Hq, case.Hkv, case.tokens
    H, h, hpw = Hq + Hkv, D // 2, GEOMETRY["qk_fwd"]["HPW"][D]
    x, w, c, s = _qk_heads(case, ns, F32)
    if defect == "key_heads_with_query_weight":
        w = ns.qw.float().expand(H, D)
    c1, c2, s1, s2 = c[..., :h], c[..., h:], s[..., :h], s[..., h:]
    r = torch.rsqrt((x * x).sum(-1, keepdim=True) / float(D) + QK_EPS) if ns.norm else torch.ones(T, H, 1)
    if rstd is not None:
        r = rstd.detach().cpu().float().reshape(T, H, 1)
    if case.form.startswith("fwd"):
        n = rbf(x * r * w)
        n1, n2 = n[..., :h], n[..., h:]
        y = torch.cat([rbf(c1 * n1) + rbf(s1 * (-n2)), rbf(c2 * n2) + rbf(s2 * n1)], -1).to(BF16)
        if defect == "second_pass_unwritten":
            y[:, hpw : 2 * hpw] = filled((1,), BF16)[0]
        got = {"y": y.reshape(T * H, D)}
        if ns.norm:
            got["rstd"] = r.reshape(T * H, 1)
        return got
    h0 = Hq if ns.konly else 0
    gq = torch.zeros(T, Hq, D) if ns.dq is None else ns.dq.float().view(T, Hq, D)
    g = torch.cat([gq, ns.dk.float().view(T, Hkv, D)], 1)
    g1, g2 = g[..., :h], g[..., h:]
    dn = torch.cat([c1 * g1 + s2 * g2, c2 * g2 - s1 * g1], -1)
    xh = x * r if ns.norm else torch.zeros_like(x)
    if ns.norm:
        dot = ((dn * w) * xh).sum(-1, keepdim=True) / float(D)
        d = r * (dn * w - xh * dot)
    else:
        d = dn
    # dw: region (wave, slot) accumulates token trips and passes in order; slots of q heads feed the first D columns, of k heads the last D
    parts = qk_parts(T, Hq, Hkv, D, case.parts)
    groups = -(-(H - h0) // hpw)
    per = parts * ROWS_PER_BLOCK
    tr = -(-T // per)
    C = torch.zeros(tr * per, groups * hpw, 2, D)
    contrib = (dn * xh)[:, h0:]
    nq = Hq - h0
    C[:T, :nq, 0] = contrib[:, :nq]
    C[:T, nq : H - h0, 1] = contrib[:, nq:]
    C = C.view(tr, parts, ROWS_PER_BLOCK, groups, hpw, 2 * D)
    acc = torch.zeros(parts, ROWS_PER_BLOCK, hpw, 2 * D)
    for i in range(tr):
        for gi in range(groups):
            acc = acc + C[i, :, :, gi]
    acc = acc.view(parts, ROWS_PER_BLOCK * hpw, 2 * D)
    partial = torch.zeros(parts, 2 * D)
    for rg in range(ROWS_PER_BLOCK * hpw):
        partial = partial + acc[:, rg]
    dw = reduce_rows_emulated(partial)
    return {"d": d[:, h0:].reshape(T * (H - h0), D).to(BF16), "dqw": dw[:D], "dkw": dw[D:]}


def qk_pack(q, k, case):
    """q [T, Hq D], k [T, Hkv D] -> [T (Hq + Hkv), D] in the reference's order"""
    T, D = case.tokens, case.D
    return torch.cat([q.view(T, case.Hq, D), k.view(T, case.Hkv, D)], 1).reshape(-1, D)


# ================================================================================================================= LayerNorm
LN_WIDTHS = (4, 192, 252, 256, 260, 764, 768, 772, 1024, 1028, 2048)
LN_ROWS = (1, 3, 5)
LN_OUTS = ("f32", "bf16", "split3")
LN_EPS = {0: 1e-5, 1: 1e-6}
LnCase = namedtuple("LnCase", "name kind rows width mode out dy_bf16 dres hot")
LN_DEFECTS = ("modes_swapped",)
LN_WRAP_BWD = 4 * LN_BWD_PARTS + 5  # 4101 rows


def _ln(kind, rows, width, mode, out="f32", dy_bf16=False, dres=False, hot=None):
    name = f"ln-{kind}-{rows}x{width}-m{mode}" + (f"-{out}" if kind == "fwd" else f"-dy{'bf16' if dy_bf16 else 'f32'}" + ("-dres" if dres else "")) + (f"-hot{hot}" if hot is not None else "")
    return LnCase(name, kind, rows, width, mode, out, dy_bf16, dres, hot)


def ln_fwd_cases():
    out = []
    for wi, w in enumerate(LN_WIDTHS):
        for mode in (0, 1):
            for oi, o in enumerate(LN_OUTS):
                out.append(_ln("fwd", LN_ROWS[(wi + mode + oi) % 3], w, mode, o))
    out += [_ln("fwd", first_wrap("layernorm_fwd"), 192, 0, "f32"), _ln("fwd", first_wrap("layernorm_fwd"), 768, 1, "bf16")]
    return out


def ln_bwd_cases():
    out = []
    for wi, w in enumerate(LN_WIDTHS):
        for mode in (0, 1):
            for bi, dy_bf16 in enumerate((False, True)):
                for ri, dres in enumerate((False, True)):
                    out.append(_ln("bwd", LN_ROWS[(wi + mode + bi + ri) % 3], w, mode, dy_bf16=dy_bf16, dres=dres))
    out += [_ln("bwd", LN_WRAP_BWD, 192, 1, dy_bf16=True, dres=True), _ln("bwd", LN_WRAP_BWD, 768, 0, dy_bf16=False, dres=True)]
    return out


def ln_structural_cases():
    return [_ln("bwd", LN_WRAP_BWD, 192, 0, dy_bf16=False, dres=False, hot=4098), _ln("bwd", LN_WRAP_BWD, 768, 1, dy_bf16=True, dres=True, hot=4098)]


@lru_cache(maxsize=4)
def ln_build(case):
    g = torch.Generator().manual_seed(seed_of(case))
    rows, width = case.rows, case.width
    x = special_rows(torch.randn(rows, width, generator=g) * 2 + 0.5, zero=False)
    sc, sh = 1 + 0.2 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    ns = SimpleNamespace(x=x, scale=sc, shift=sh, dy=None, dres=None, eps=LN_EPS[case.mode])
    if case.kind == "bwd":
        dy = torch.randn(rows, width, generator=g)
        if case.hot is not None:
            keep = dy[case.hot].clone()
            dy.zero_()
            dy[case.hot] = keep
        ns.dy = dy.to(BF16) if case.dy_bf16 else dy
        ns.dres = torch.randn(rows, width, generator=g) if case.dres else None
    return ns


def _ln_stats(x, mode, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return mu, var, (1.0 / (var.sqrt() + eps) if mode == 0 else torch.rsqrt(var + eps))


def ln_reference(case, ns, dt, mode=None):
    mode = case.mode if mode is None else mode
    x, sc, sh = ns.x.to(dt), ns.scale.to(dt), ns.shift.to(dt)
    mu, var, inv = _ln_stats(x, mode, ns.eps)
    xm = x.abs() + x.abs().mean(-1, keepdim=True)  # |x| + the |x_i| / width that the mean adds
    if case.kind == "fwd":
        y = sc * ((x - mu) * inv) + sh
        R = {"f32": 0, "bf16": 1, "split3": SPLIT3_LO}[case.out]
        return {"y": out(y, sc.abs() * inv * xm + sh.abs(), R, "row"),
                "mean": out(mu, x.abs().mean(-1, keepdim=True), 0, "row"),
                "rsig": out(inv, inv * (xm * xm).mean(-1, keepdim=True) / var, 0, "row")}
    dy = ns.dy.to(dt)
    n, nm = (x - mu) * inv, xm * inv
    dn = dy * sc
    sos = (1.0 / inv) / (1.0 / inv - ns.eps) if mode == 0 else torch.ones_like(inv)
    dx = inv * (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True) * sos)
    mag = inv * (dn.abs() + dn.abs().mean(-1, keepdim=True) + nm * (dn.abs() * nm).mean(-1, keepdim=True) * sos)
    if ns.dres is not None:
        dx, mag = dx + ns.dres.to(dt), mag + ns.dres.to(dt).abs()
    return {"dx": out(dx, mag, 0, "row"), "dscale": out(col((dy * n).sum(0)), col((dy.abs() * nm).sum(0)), 0, "column"),
            "dshift": out(col(dy.sum(0)), col(dy.abs().sum(0)), 0, "column")}


@lru_cache(maxsize=4)
def ln_exact(case):
    ns = ln_build(case)
    return finish(ln_reference(case, ns, F64), ln_reference(case, ns, F32))


def ln_autograd(case):
    """fp64 autograd of the forward formula -> dx, dscale, dshift: what validates the closed form of ``ln_reference``"""
    ns = ln_build(case)
    x, sc, sh = ns.x.double().requires_grad_(True), ns.scale.double().requires_grad_(True), ns.shift.double().requires_grad_(True)
    mu, var, inv = _ln_stats(x, case.mode, ns.eps)
    (sc * ((x - mu) * inv) + sh).backward(ns.dy.double())
    return x.grad + (0 if ns.dres is None else ns.dres.double()), sc.grad, sh.grad


def ln_split3(y, width):
    """bf16 [rows, 3 width] = [hi | lo | hi] -> (hi + lo in fp64, the third block equals the first bit for bit)"""
    hi, lo, hi2 = y[:, :width], y[:, width : 2 * width], y[:, 2 * width :]
    return hi.double() + lo.double(), same_bits(hi.contiguous(), hi2.contiguous())


def ln_emulate(case, defect=None):
    """fp32 in the kernel's order of operations; defect modes_swapped: mode 1's formula under mode 0 and the other way round"""
    assert defect is None or defect in LN_DEFECTS
    ns = ln_build(case)
    mode = 1 - case.mode if defect == "modes_swapped" else case.mode
    x, sc, sh, width = ns.x, ns.scale, ns.shift, case.width
    eps = torch.tensor(ns.eps, dtype=F32)
    mu = x.sum(-1, keepdim=True) / float(width)
    var = ((x - mu) * (x - mu)).sum(-1, keepdim=True) / float(width)
    inv = 1.0 / (var.sqrt() + eps) if mode == 0 else torch.rsqrt(var + eps)
    if case.kind == "fwd":
        o = sc * ((x - mu) * inv) + sh
        if case.out == "bf16":
            y = o.to(BF16)
        elif case.out == "split3":
            hi = o.to(BF16)
            y = torch.cat([hi, (o - hi.float()).to(BF16), hi], 1)
        else:
            y = o
        return {"y": y, "mean": mu, "rsig": inv}
    g = ns.dy.float()
    n, dn = (x - mu) * inv, g * sc
    s1, s2 = dn.sum(-1, keepdim=True) / float(width), (dn * n).sum(-1, keepdim=True) / float(width)
    sos = (1.0 / inv) / (1.0 / inv - eps) if mode == 0 else torch.ones_like(inv)
    dx = inv * (dn - s1 - n * s2 * sos)
    if ns.dres is not None:
        dx = dx + ns.dres
    both = reduce_rows_emulated(partition_sum(torch.cat([g * n, g], 1), blocks("layernorm_bwd", case.rows)))
    return {"dx": dx, "dscale": both[:width], "dshift": both[width:]}


def ln_got(case, got):
    """the outputs as ``judge`` takes them: a split3 forward is judged as hi + lo"""
    if case.kind == "fwd" and case.out == "split3":
        got = dict(got)
        got["y"] = ln_split3(got["y"].detach().cpu(), case.width)[0]
    return got


# ================================================================================================================= SwiGLU and GELU
# the overflow pair and the largest values first: the smallest GELU case holds eight elements
SPECIALS = (89.0, -89.0, 1000.0, -1000.0, 0.0, -0.0, 2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, 10.0, -10.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0)
ActCase = namedtuple("ActCase", "name op tokens F kind n")
ACT_DEFECTS = ("halves_exchanged",)
ONE_TRIP = GEOMETRY["swiglu"]["cap"] * GEOMETRY["swiglu"]["threads"]  # 524,288 vectors
SWIGLU_WRAP = (1366, 3080)  # 525,910 vectors
GELU_K0, GELU_A = 0.7978845608028654, 0.044715


def act_cases():
    out = [ActCase(f"swiglu-{t}x{F}", "swiglu", t, F, None, None) for t, F in ((5, 8), (1, 72), (3, 3072), (5, 3080), SWIGLU_WRAP)]
    for kind in (0, 1):
        out += [ActCase(f"gelu{kind}-n{n}", "gelu", None, None, kind, n) for n in (8, 8 * 257, 8 * (ONE_TRIP + 257))]
    return out


def plant_specials(t2d):
    """the special values down column 0 of [rows, cols], continued in the next columns when the rows run out; as many as the tensor holds"""
    rows, cols = t2d.shape
    for i, v in enumerate(SPECIALS[: rows * cols]):
        t2d[i % rows, i // rows] = v
    return t2d


@lru_cache(maxsize=2)
def act_build(case):
    g = torch.Generator().manual_seed(seed_of(case))
    if case.op == "swiglu":
        t, F = case.tokens, case.F
        gu = special_rows(torch.randn(t, 2 * F, generator=g) * 2)
        plant_specials(gu[:, F:])
        return SimpleNamespace(gu=gu.to(BF16), da=torch.randn(t, F, generator=g).to(BF16))
    x = (torch.randn(case.n // 8, 8, generator=g) * 2)
    x[-1] = 0.0  # a padding vector
    plant_specials(x)
    return SimpleNamespace(x=x.to(BF16), dy=torch.randn(case.n // 8, 8, generator=g).to(BF16))


def act_reference(case, ns, dt):
    one = torch.ones((), dtype=dt)
    if case.op == "swiglu":
        F = case.F
        u, g, d = ns.gu[:, :F].to(dt), ns.gu[:, F:].to(dt), ns.da.to(dt)
        sg = torch.sigmoid(g)
        a, du = u * (g * sg), d * g * sg
        dg = d * u * sg * (1 + g * (1 - sg))
        dgm = (d * u * sg).abs() * (1 + (g * (1 - sg)).abs())
        return {"a": out(a, a.abs(), 2, "token", tiny=TINY * torch.maximum(one, (g * u).abs())),
                "du": out(du, du.abs(), 1, "token", tiny=TINY * torch.maximum(one, (d * g).abs())),
                "dg": out(dg, dgm, 1, "token", tiny=TINY * torch.maximum(one, (d * u).abs() * (1 + g.abs())))}
    x, dy = ns.x.to(dt), ns.dy.to(dt)
    if case.kind == 0:
        e = torch.erf(x * 0.70710678118654752440)
        y, ym = x * 0.5 * (1 + e), (0.5 * x).abs() * (1 + e.abs())
        p = x * 0.3989422804014327 * torch.exp(-0.5 * x * x)
        gr, grm = 0.5 * (1 + e) + p, 0.5 * (1 + e.abs()) + p.abs()
    else:
        th = torch.tanh(GELU_K0 * (x + GELU_A * x * x * x))
        y, ym = 0.5 * x * (1 + th), (0.5 * x).abs() * (1 + th.abs())
        q = 0.5 * x * GELU_K0 * (1 + 3 * GELU_A * x * x)
        gr, grm = 0.5 * (1 + th) + q * (1 - th * th), 0.5 * (1 + th.abs()) + q.abs() * (1 + th * th)
    xa = torch.maximum(one, x.abs())
    return {"y": out(y, ym, 1, "vector", tiny=TINY * xa), "dx": out(dy * gr, dy.abs() * grm, 1, "vector", tiny=TINY * xa * torch.maximum(one, dy.abs()))}


@lru_cache(maxsize=2)
def act_exact(case):
    ns = act_build(case)
    return finish(act_reference(case, ns, F64), act_reference(case, ns, F32))


def act_emulate(case, defect=None, sigmoid_scale=1.0):
    """SwiGLU: a = bf16(u * bf16(g * sigmoid(g))), the gradients in fp32 with one rounding; GELU: fp32 with one rounding.  a_alt: the forward with the
    inner rounding point one bf16 step up and one step down (see ``steps_from``).  sigmoid_scale: a relative perturbation of the fp32 sigmoid (what a
    hardware exp and reciprocal do to it).  Defect halves_exchanged: the SwiGLU kernels read g where u lies and u where g lies."""
    assert defect is None or defect in ACT_DEFECTS
    ns = act_build(case)
    if case.op == "swiglu":
        F = case.F
        u, g, d = ns.gu[:, :F].float(), ns.gu[:, F:].float(), ns.da.float()
        if defect == "halves_exchanged":
            u, g = g, u
        sg = 1.0 / (1.0 + torch.exp(-g)) * sigmoid_scale
        s = (g * sg).to(BF16)  # the inner rounding point: silu(g) is a bf16 tensor
        return {"a": (u * s.float()).to(BF16), "a_alt": [(u * bf16_step(s, k).float()).to(BF16) for k in (1, -1)], "du": (d * g * sg).to(BF16), "dg": (d * u * sg * (1.0 + g * (1.0 - sg))).to(BF16)}
    ref = act_reference(case, ns, F32)
    return {"y": ref["y"].ref.to(BF16), "dx": ref["dx"].ref.to(BF16)}


# ----------------------------------------------------------------------------------------------------------------- what must be judged, from the case alone
def expected_units(case):
    if isinstance(case, RmsCase):
        return case.rows * (2 if case.want_rstd else 1) if case.kind == "fwd" else case.rows + case.width
    if isinstance(case, RedCase):
        return case.n
    if isinstance(case, QkCase):
        H = case.Hq + case.Hkv
        if case.form.startswith("fwd"):
            return case.tokens * H * (2 if case.form == "fwd" else 1)
        return case.tokens * (case.Hkv if case.form == "bwd_k" else H) + 2 * case.D
    if isinstance(case, LnCase):
        return 3 * case.rows if case.kind == "fwd" else case.rows + 2 * case.width
    return 3 * case.tokens if case.op == "swiglu" else 2 * (case.n // 8)


FAMILIES = {  # name -> (cases, exact, emulate)
    "rmsnorm": (lambda: rms_fwd_cases() + rms_bwd_cases() + rms_structural_cases(), rms_exact, rms_emulate),
    "reduce_rows": (red_cases, red_exact, red_emulate),
    "qknorm_rope": (lambda: qk_cases() + qk_structural_cases(), qk_exact, qk_emulate),
    "layernorm": (lambda: ln_fwd_cases() + ln_bwd_cases() + ln_structural_cases(), ln_exact, lambda case, defect=None: ln_got(case, ln_emulate(case, defect))),
    "swiglu_gelu": (act_cases, act_exact, act_emulate),
}


# ----------------------------------------------------------------------------------------------------------------- measured figures
# family -> (smallest c, largest c) over all its cases on an x86-64 host with torch's fp32 CPU kernels, as test_row_sweep_cpu.py prints them, and the
# largest error / bound seen on an MI355X, as test_row_sweep_gpu.py prints it.  A record, not a bound: nothing asserts against it.
MEASURED = {
    "rmsnorm": (4.631e-06, 1.713e-05, 0.497),
    "reduce_rows": (C_FLOOR, 1.911e-05, 0.496),
    "qknorm_rope": (C_FLOOR, 1.891e-05, 0.498),
    "layernorm": (1.926e-06, 1.523e-05, 0.497),
    "swiglu_gelu": (C_FLOOR, 6.257e-05, 0.844),
}
