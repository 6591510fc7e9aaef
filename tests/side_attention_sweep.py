"""The fp64 sweep of the attention families on the plain 32-key tile layer (csrc/attn_tile32.h): ``band_*`` of csrc/attention_band.hip (behind
mi355_swa_attn_* and mi355_sink_attn_*), ``ga_*`` of csrc/attention_generic.hip (mi355_attn_generic_*, and mi355_attn_dropout_* at p = 0) and
``mla_*`` of csrc/deepseek.hip.  Case tables, operand builders, reference adapters, an fp32 emulation of the kernels' rounding points, the per-block
judgement and the coverage predicates, shared by test_side_attention_sweep_cpu.py and test_side_attention_sweep_gpu.py.
TEST INFRASTRUCTURE ONLY.

Judgement.  attention_sweep.py's, not a copy: every output [B, H, S, .] is cut into blocks of 32 consecutive tokens per (sample, head) (a ragged tail
joins the block before it), and every block and the whole tensor must satisfy rel_l2(kernel, exact) <= max(1.5 x floor, cap), caps 4e-3 for o and 8e-3
for every gradient (``attention_sweep.judge_tensor``).  ``exact`` is the family's plain-torch restatement on the operands upcast to fp64, ``floor`` the
same restatement on the bf16 operands as given: gemma3_oracle.swa_attention(_bwd), mimo_oracle.sink_attention(_bwd), deepseek_oracle.mla_attention
with the shared rotary key handed in as a per-head leaf [B, H, S, Dr] (autograd then yields each head's share, what the kernel writes to
dk_rope_heads; test_side_attention_sweep_cpu.py asserts that the shares sum to mla_attention_bwd's gradient), and ``ga_attention`` below (the
quirk allowed(i, j) = j <= i OR key j is padding; plain causal or every key for the PLAIN semantics).  Judged: o, dq, dk, dv; for MLA o, dq_nope,
dq_rope, dk_nope, dk_rope_heads (as [B, Hq, S, Dr]) and dv; lse on every row within LSE_TOL of the fp64 log-sum-exp (these kernels scale the fp32
scores and fold nothing into a bf16 operand: the tuned sweep's one-key exception is not used); dsink per head under the 1.5x rule as
test_mimo_gpu.py applies it (1.5 x floor, plus 2e-3 where the floor is below 1e-2; 1e-6 absolute where the exact value is zero).  A NaN or Inf fails
the case and names (sample, head, token, feature).  No block is left out: ``judge_case`` counts the blocks it judged and the blocks there are, and
the tests assert both against ``blocks_of`` (computed from the case alone).

Rows with no relative distance.  Without a sink a query that sees ONE key has dq = 0 exactly (the first query of a sequence; every query at W = 1 or
S = 1), and a key whose every query is such a row has dk = 0 (every key at W = 1 or S = 1): ``attention_sweep.one_key_bounds`` on the case's
allowed-pairs matrix bounds them by one rounding of o entering delta.  With a sink no row is a one-key row (the sink is a second term of its
softmax) and no rule is handed over, so a zero exact block there fails as "no rule covers it".  The sink of -30000 is the one exception: exp(z - s)
is exactly 0 in fp64 too, the exact values are those without a sink, and the one-key rules apply.

Few-key blocks (W in {1, 2}, the first rows of every sequence).  The fp32 emulation below (bf16 operands, fp32 scores and statistics, P and dS rounded
to bf16 before they enter a product, one bf16 rounding of every output, fp32 dk_rope_heads / dsink / lse) was run through the plain bound on every
block of every case before a GPU saw one.  It stays inside everywhere except in the two classes of the next paragraph, one of which is a few-key
class (a window of one with a live sink); every other few-key block -- W = 2, W = 1 without a sink, the first rows of a sequence inside their block --
keeps the plain caps.  (Why the tuned sweep's S = 1 exception for o does not come back here: these kernels measure every row against its running
maximum, so a one-key row has P = 1 exactly, l = 1 and o = v_j bit for bit.)

Derived bounds.  Two classes where the kernels' documented rounding points (P rounded to bf16 before P V, ONE rounding of o, delta = dO . o read from
that rounded o) cannot meet the plain numbers; the honest emulation showed both on the CPU before a GPU saw a case, each class gets the bound its
rounding points give, and nothing else is widened.  (The bf16 restatement does not have these errors -- its softmax backward sums p (dO . v) without
going through a rounded o -- so its floor is small there.)  Half a bf16 ulp is at most 2^-8 of the value.
  1. dsink per head.  dz_h = - sum_{b,i} w_i delta_i, w_i = exp(z_h - lse_i): a signed sum over B S rows that cancels to the size of sqrt(B S) terms,
     while every delta_i carries the roundings of its o_i: one independent rounding per element o_id (at most 2^-8 |o_id|, variance at most a third of
     its square) and, in front of it, one per P_ij (at most 2^-8 p_ij, moving delta_i by that times dP_ij = dO_i . v_j).  So the error of dz_h is a sum
     of independent terms with sigma_h^2 <= 2^-16 / 3 sum_i w_i^2 (sum_d (dO_id o_id)^2 + sum_j p_ij^2 dP_ij^2) (``dsink_sigma``), relative to |dz_h|
     anything from 1e-3 up, far above the restatement's floor (about 5e-4) whenever the sum happens to cancel.  A head passes when it meets the 1.5x
     rule OR |error| <= DSINK_SIGMAS x sigma_h: 4 sigma, because the three tables hold about 330 judged heads and a sum of at least 64 independent
     bounded terms passes 4 sigma with probability 6e-5.  The emulation's worst is 1.83 sigma (median 0.40: the model is an upper bound, not a fit); 21
     of its 324 heads miss the 1.5x rule alone, by up to a factor 6.
     A head beyond 4 sigma is a finding about the kernel (or about this model), to be traced to its rounding point: DSINK_SIGMAS is not a dial.
  2. dq and dk where every softmax is ONE key and a live sink (W = 1 or S = 1 with a sink other than -30000).  P = 1 and l = 1 in the loop, the merge
     gives o_i = bf16(p_i v_i) with p_i = 1 / (1 + exp(z - s_ii)): one rounding, nothing to average over.  The kernels round t_i = scale p_i (dP_i -
     delta_i) to bf16 as dS, with delta_i = dO_i . o_i read from the rounded o, while the exact dP_i - delta_i = (1 - p_i) dP_i is small wherever the
     sink is weak: the rounding of o enters by cancellation.  All roundings are independent and uniform over one ulp (variance ulp^2 / 12, the ulp of
     the exact value: ``rounding_variance``): var(delta_i) = sum_e dO_ie^2 var(o_ie); the rounded dS of row i has variance u_i = scale^2 p_i^2
     var(delta_i) + var(t_i); an element has var(dq_id) = k_id^2 u_i + var of its own output rounding, and var(dk_jd) is the same with q_jd^2 u
     summed over the group's heads.  A block's squared error norm has the sum of these as its expectation, sigma^2 (``one_key_sink_sigma``).  This
     is a fit, not an upper bound: over the class's 340 blocks the emulation's error norm is 0.97 sigma in the median and 1.40 sigma at worst.  The
     cap of a block is ONE_KEY_SINK_SIGMAS = 2 sigma over the block's norm, and the plain 8e-3 wherever that is no more (208 of the 340 blocks keep
     the plain cap).  Why 2: the squared norm is a sum over 32 rows of independent terms, each itself a sum over at least 32 roundings, plus 32 D
     output roundings; 2 sigma means 4 times its expectation, which a sum of 32 comparable squares passes with probability below 1e-9 and one of
     only 8 effective rows with 9e-5.  Four blocks of the emulation exceed the plain bound, the worst at 1.19e-2 against 8e-3: 0.70 of its cap.
     test_side_attention_sweep_cpu.py asserts these figures from below and from above.  A block beyond 2 sigma is a finding, not a cue to raise the
     multiple.  Rows of this kind inside other blocks (the first query of every sequence) vanish in their block's norm.

Operands.  bf16 N(0, 1), seeded from the case; sink logits N(0, 1) per head rounded to bf16, and per (D, DV) pair one case with a sink far below
every score (-30000) and one far above (+30), both placed behind a walk of several tiles with skipped tiles on both sides and a row whose first
tile holds none of its keys (S >= 129).  The GPU tests pre-fill every caller-provided output with NaN (the fp32 ones too) and put 32 rows of
NaN behind the last token of every operand, inside the same allocation: a tile row past S that is not zero-filled (``load_tile``'s rows >= rows_valid)
enters an MFMA as 0 x NaN and is seen.  ("One row of a ragged last tile read as its neighbour instead of zero" changes no value when the neighbour is
finite -- every use of such a row is also masked by key < S or query < S -- so the NaN tail is what makes that fault visible; the emulation's planted
fault reads the same neighbour, and "caught" there means no more than that the judgement sees the NaN.  On the GPU the protection is those tail rows
alone, and it reaches only the rows read behind the LAST sample of a case with S % 32 != 0; behind an earlier sample lies the next one's finite data.)

Geometry, quoted from the three files.  A workgroup is 256 threads = 4 waves and owns 128 rows (queries in the forward and dQ pass, keys in the
dK/dV pass); a wave owns 32 of them (q0 = qb + 32 wave, k0 = kb + 32 wave); a tile is 32 keys (or 32 queries in the key-major pass).
  band forward / dQ:  kfirst = max(qb - W + 1, 0);  for kt in kfirst / 32 .. qlast / 32, qlast = min(qb + 127, S - 1);  a wave skips the tile when
      q0 >= S || key0 > q0 + 31 || key0 + 31 + W <= q0.
  band dK/dV:  qend = min(klast + W - 1, S - 1), klast = min(kb + 127, S - 1);  for hq in the group, for qt in kb / 32 .. qend / 32;  a wave skips when
      k0 >= S || qs + 31 < k0 || qs >= k0 + 31 + W.
  ga:  all_keys = PLAIN ? !causal : key_mask != nullptr;  ntiles = all_keys ? (S + 31) / 32 : qlast / 32 + 1;  skip when !all_keys && key0 > q0 + 31;
      dK/dV in NP = 2 slices of 128 columns at D = 256 (blockIdx.x = key_block * NP + slice, c0 = 32 (slice * NDT + dt)).
  mla:  kt in 0 .. qlast / 32, skip when q0 >= S || key0 > q0 + 31;  dK/dV over qt in kb / 32 .. (S - 1) / 32, NP = 2 at (128, 64) (3 dK^T and 2 dV^T
      tiles per slice); dK^T tiles at columns >= Dn go to the fp32 scratch dk_rope_heads.
``band_branches`` / ``ga_branches`` / ``mla_branches`` compute from a case alone which of these branches it takes; the CPU test asserts that every
branch is taken by a case of every (D, DV) pair, every D and every (Dn, Dr) that has it.

Tables.  band: S in BAND_S x W in (1, 2, 31, 32, 33, 64, 96, 127, 128, 129, S - 1, S) up to S plus one W > S (S + 1 or 2^40 in turn), every cell with
two of the six (D, DV) pairs in turn; heads, sink off / on and the entry point (swa_attn_* / sink_attn_* for DV = D without a sink) rotate with the
pair's own case count.  ga: SWEEP_S x D in (32, 64, 128, 256), heads and the five modes rotating.  mla: SWEEP_S x ((64, 32), (128, 64)), Hq and packed /
sliced operands rotating.  B = 2 up to S = 200, else 1.

MEASURED holds the worst block ratio (value / bound) per family and tensor: of the emulation on an x86-64 host (test_side_attention_sweep_cpu.py
prints them again on every run) and of the kernels on an MI355X (test_side_attention_sweep_gpu.py prints them): all 224 + 64 + 32 cases pass, no
ratio above 0.75.  The two columns agree to the third digit almost everywhere: the emulation's rounding points are the kernels', and the worst blocks
are few-key blocks, where a handful of roundings decide the figure.  lse is within 1e-5 of fp64 (0.000 of its tolerance).
"""

import math
import zlib
from collections import namedtuple
from functools import lru_cache

import torch

import attention_sweep as A
import deepseek_oracle as DO
import gemma3_oracle as GO
import mimo_oracle as MO
from attention_sweep import BF16, CAP, LSE_TOL, block_edges, judge_tensor, n_blocks, one_key_bounds  # noqa: F401  (the project's judgement, not a copy)

GRAD_CAP = CAP["dq"]
SINK_LOW, SINK_HIGH = -30000.0, 30.0
DSINK_ZERO_TOL = 1e-6  # test_gemma3_gpu.judge: where the exact value is zero
DSINK_SIGMAS = 4.0  # "Derived bounds" 1
ONE_KEY_SINK_SIGMAS = 2.0  # "Derived bounds" 2
TAIL_ROWS = 32  # rows of NaN behind the last token of every GPU operand

# worst ratio (value / bound) per tensor over the family's table: (emulation on the CPU, kernels on an MI355X)
MEASURED = {
    "band": {"o": (0.513, 0.513), "dq": (0.747, 0.747), "dk": (0.616, 0.616), "dv": (0.371, 0.371), "lse": (0.000, 0.000), "dsink": (0.457, 0.456)},
    "ga": {"o": (0.481, 0.481), "dq": (0.598, 0.598), "dk": (0.392, 0.392), "dv": (0.342, 0.342), "lse": (0.000, 0.000)},
    "mla": {"o": (0.471, 0.471), "dq_nope": (0.399, 0.399), "dq_rope": (0.399, 0.399), "dk_nope": (0.402, 0.402), "dk_rope_heads": (0.389, 0.389),
            "dv": (0.331, 0.331), "lse": (0.000, 0.000)},
}

# ----------------------------------------------------------------------------------------------------------------- the tables
BandCase = namedtuple("BandCase", "B S Hq Hkv D DV W sink entry")  # sink: None | "rand" | "low" | "high"; entry: "swa" | "sink"
GaCase = namedtuple("GaCase", "B S Hq Hkv D mode")
MlaCase = namedtuple("MlaCase", "B S Hq Dn Dr sliced")

BAND_S = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160, 257, 385)
BAND_W = (1, 2, 31, 32, 33, 64, 96, 127, 128, 129)
W_HUGE = 2 ** 40
BAND_PAIRS = ((32, 32), (64, 32), (64, 64), (128, 64), (128, 128), (192, 128))  # (32, 32): the windowed entry points only
BAND_HEADS = ((2, 1), (2, 2), (3, 3), (6, 2), (6, 1))
GA_D = (32, 64, 128, 256)
GA_HEADS = ((2, 1), (4, 4), (8, 2))
GA_MODES = ("quirk", "quirk-right", "quirk-holes", "plain-causal", "plain-full")
MLA_DIMS = ((64, 32), (128, 64))
MLA_HEADS = (1, 2, 3)
PAIRS_PER_CELL = 2


def _batch(S):
    return 2 if S <= 200 else 1


def band_windows(S, si):
    """The windows of one length: the listed ones up to S (values that coincide after the host's clamp to S dropped) and one W > S."""
    return sorted({w for w in BAND_W + (S - 1, S) if 1 <= w <= S}) + [(S + 1, W_HUGE)[si % 2]]


@lru_cache(maxsize=None)
def band_cases():
    out, count, plain = [], {}, {}
    cell = 0
    for si, S in enumerate(BAND_S):
        for W in band_windows(S, si):
            for r in range(PAIRS_PER_CELL):
                pair = BAND_PAIRS[(cell + r * (1 + (cell // 6) % 5)) % 6]
                n = count[pair] = count.get(pair, -1) + 1
                Hq, Hkv = BAND_HEADS[n % 5]
                sink, entry = None, "swa"
                if pair != (32, 32):
                    if n % 2:
                        sink, entry = "rand", "sink"
                    else:
                        p = plain[pair] = plain.get(pair, -1) + 1
                        entry = "swa" if pair[0] == pair[1] and p % 2 == 0 else "sink"
                out.append(BandCase(_batch(S), S, Hq, Hkv, pair[0], pair[1], W, sink, entry))
            cell += 1
    # one sink far above and one far below every score per pair, each behind a walk that has every feature of the forward's loop: the first and
    # the second case of the pair with a sink whose workgroups start their walk in an earlier 128-block, whose waves skip tiles on both sides and
    # which has a row that meets its first tile with none of its keys in it
    for pair in BAND_PAIRS[1:]:
        walks = [i for i, c in enumerate(out) if (c.D, c.DV) == pair and c.sink and all(band_branches(c)[b] for b in BAND_BRANCHES[:4])]
        out[walks[0]], out[walks[1]] = out[walks[0]]._replace(sink="high"), out[walks[1]]._replace(sink="low")
    return tuple(out)


@lru_cache(maxsize=None)
def ga_cases():
    return tuple(GaCase(_batch(S), S, *GA_HEADS[(si + di) % 3], D, GA_MODES[(si + 2 * di) % 5]) for si, S in enumerate(A.SWEEP_S) for di, D in enumerate(GA_D))


@lru_cache(maxsize=None)
def mla_cases():
    return tuple(MlaCase(_batch(S), S, MLA_HEADS[(si + di) % 3], Dn, Dr, bool((si + di) % 2)) for si, S in enumerate(A.SWEEP_S)
                 for di, (Dn, Dr) in enumerate(MLA_DIMS))


def case_id(c):
    if isinstance(c, BandCase):
        return f"S{c.S}-W{'2^40' if c.W == W_HUGE else c.W}-H{c.Hq}x{c.Hkv}-D{c.D}x{c.DV}-{c.sink or 'nosink'}-{c.entry}"
    if isinstance(c, GaCase):
        return f"S{c.S}-H{c.Hq}x{c.Hkv}-D{c.D}-{c.mode}"
    return f"S{c.S}-H{c.Hq}-D{c.Dn}+{c.Dr}-{'sliced' if c.sliced else 'packed'}"


def family_of(c):
    return "band" if isinstance(c, BandCase) else "ga" if isinstance(c, GaCase) else "mla"


NAMES = {"band": ("o", "dq", "dk", "dv"), "ga": ("o", "dq", "dk", "dv"), "mla": ("o", "dq_nope", "dq_rope", "dk_nope", "dk_rope_heads", "dv")}


def blocks_of(c):
    """The number of 32-token blocks of all judged tensors, from the case alone."""
    if isinstance(c, MlaCase):
        return 6 * n_blocks(c.B, c.Hq, c.S)
    return 2 * n_blocks(c.B, c.Hq, c.S) + 2 * n_blocks(c.B, c.Hkv, c.S)


# ----------------------------------------------------------------------------------------------------------------- operands and masks
def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(repr(tuple(c)).encode()))


def band_operands(c):
    """-> (q [B, Hq, S, D], k [B, Hkv, S, D], v [B, Hkv, S, DV], do [B, Hq, S, DV], sink fp32 [Hq] of bf16 values or None)"""
    g = _gen(c)
    rn = lambda h, d: torch.randn(c.B, h, c.S, d, generator=g).to(BF16)
    q, k, v, do = rn(c.Hq, c.D), rn(c.Hkv, c.D), rn(c.Hkv, c.DV), rn(c.Hq, c.DV)
    z = torch.randn(c.Hq, generator=g)
    if c.sink is None:
        return q, k, v, do, None
    z = z if c.sink == "rand" else torch.full((c.Hq,), SINK_LOW if c.sink == "low" else SINK_HIGH)
    return q, k, v, do, z.to(BF16).float()


def ga_operands(c):
    g = _gen(c)
    rn = lambda h: torch.randn(c.B, h, c.S, c.D, generator=g).to(BF16)
    return rn(c.Hq), rn(c.Hkv), rn(c.Hkv), rn(c.Hq)


def mla_operands(c):
    """-> (q_nope, q_rope, k_nope [B, H, S, .], k_rope [B, S, Dr], v, do)"""
    g = _gen(c)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF16)
    B, H, S = c.B, c.Hq, c.S
    return rn(B, H, S, c.Dn), rn(B, H, S, c.Dr), rn(B, H, S, c.Dn), rn(B, S, c.Dr), rn(B, H, S, c.Dn), rn(B, H, S, c.Dn)


def band_allowed(S, W):
    """bool [S, S]: query i sees key j iff i - W < j <= i"""
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return (j <= i) & (j > i - W)


def ga_key_mask(c):
    return A.key_mask(c.mode[6:], c.B, c.S) if c.mode in ("quirk-right", "quirk-holes") else None


def allowed_of(c):
    """bool [B, S, S]: the pairs (query, key) of the case that see each other."""
    S = c.S
    tril = torch.ones(S, S, dtype=torch.bool).tril_()
    if isinstance(c, BandCase):
        a = band_allowed(S, c.W)
    elif isinstance(c, MlaCase) or c.mode in ("quirk", "plain-causal"):
        a = tril
    elif c.mode == "plain-full":
        a = torch.ones(S, S, dtype=torch.bool)
    else:  # the upstream quirk: a padded key is visible to every query
        return tril[None] | ~ga_key_mask(c).bool()[:, None, :]
    return a[None].expand(c.B, S, S)


# ----------------------------------------------------------------------------------------------------------------- the restatements
def ga_attention(q, k, v, allowed, exact=False):
    """SDPA on the boolean mask ``allowed`` [B, S, S] (True = attend): q [B, Hq, S, D], k / v [B, Hkv, S, D] -> (o, lse [B, Hq, S]); bf16 ops on
    bf16 tensors, fp64 with ``exact``."""
    rep = q.shape[1] // k.shape[1]
    q, k, v = (t.double() if exact else t for t in (q, k, v))
    k, v = k.repeat_interleave(rep, dim=1), v.repeat_interleave(rep, dim=1)
    s = (q @ k.mT) * q.shape[-1] ** -0.5
    s = s.masked_fill(~allowed[:, None], -torch.inf)
    return torch.softmax(s, dim=-1) @ v, torch.logsumexp(s.double() if exact else s.float(), dim=-1)


def ga_attention_bwd(q, k, v, do, allowed, exact=False):
    leaves = [(t.double() if exact else t).detach().requires_grad_(True) for t in (q, k, v)]
    o, _ = ga_attention(*leaves, allowed, exact)
    return torch.autograd.grad(o, leaves, do.double() if exact else do)


def reference(c, ops):
    """-> (exact, floor): dicts of the family's tensors [B, H, S, .], lse [B, Hq, S] and (band with a sink) dsink [Hq]."""
    out = []
    for exact in (True, False):
        if isinstance(c, BandCase):
            q, k, v, do, z = ops
            if c.entry == "swa":
                o, lse = GO.swa_attention(q, k, v, c.W, exact)
                dq, dk, dv = GO.swa_attention_bwd(q, k, v, do, c.W, exact)
                dz = None
            else:
                o, lse = MO.sink_attention(q, k, v, c.W, z, exact)
                dq, dk, dv, dz = MO.sink_attention_bwd(q, k, v, do, c.W, z, exact)
            out.append(dict(o=o.detach(), lse=lse.detach(), dq=dq, dk=dk, dv=dv, dsink=dz))
        elif isinstance(c, GaCase):
            q, k, v, do = ops
            al = allowed_of(c)
            o, lse = ga_attention(q, k, v, al, exact)
            dq, dk, dv = ga_attention_bwd(q, k, v, do, al, exact)
            out.append(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv))
        else:
            qn, qr, kn, kr, v, do = ops
            dt = torch.float64 if exact else None
            cast = lambda t: t.double() if exact else t
            leaves = [cast(t).detach().requires_grad_(True) for t in (qn, qr, kn, kr[:, None].expand(-1, c.Hq, -1, -1).contiguous(), v)]
            o, lse = DO.mla_attention(*leaves, dtype=dt)
            g = torch.autograd.grad(o, leaves, cast(do))
            out.append(dict(o=o.detach(), lse=lse.detach(), dq_nope=g[0], dq_rope=g[1], dk_nope=g[2], dk_rope_heads=g[3], dv=g[4]))
    return out[0], out[1]


# ----------------------------------------------------------------------------------------------------------------- the emulation
FAULTS = {
    "window one too wide": "band", "window one too narrow": "band", "first tile of a row's band dropped": "band", "sink left out of l": "band",
    "sink multiplied by the scale": "band", "sink absent from the backward's lse": "band", "query head mapped to h % Hkv": "band",
    "last partial row of dsink dropped": "band",
    "quirk dropped, padded keys masked": "ga", "PLAIN full run as causal": "ga", "second dK/dV slice at D = 256 unstored": "ga",
    "rope half of the score dropped": "mla", "k_rope not shared": "mla", "second dK/dV slice at (128, 64) unstored": "mla",
    "ragged tile row read as its neighbour": "all",
}


def _bf(t):
    return t.to(BF16).float()


def _core(q, k, v, do, allowed, scale, sink=None, fault=None, qs=None, ks=None, v_next=None):
    """attention_sweep.emulate(fold=False) with the sink term and dV / dK per QUERY head: q, k [B, H, S, DK] fp32 (k already repeated per query head),
    v, do [B, H, S, DV], allowed bool [B, 1, S, S]; ``qs`` / ``ks``: what the score product reads, where a planted fault makes that differ.
    Rounding points: bf16 operands, fp32 scores and statistics, P rounded to bf16 before P V, dS (scale included, as the kernels apply it) rounded to
    bf16 before dS K and dS^T Q, P rounded before P^T dO, one bf16 rounding of o (the backward's delta reads that o); everything else fp32."""
    s = ((q if qs is None else qs) @ (k if ks is None else ks).mT) * scale
    sm = s.masked_fill(~allowed, -torch.inf)
    m = sm.max(dim=-1, keepdim=True).values
    p = torch.exp(sm - m)
    l = p.sum(dim=-1, keepdim=True)
    acc = _bf(p) @ v
    if v_next is not None:
        acc = acc + 0.0 * v_next  # FAULT: the tile row behind the last key holds the next row of the buffer; its P is 0
    m0, l0, z = m, l, None
    if sink is not None:  # merged behind the loop, like a last tile
        z = sink.view(1, -1, 1, 1) * (scale if fault == "sink multiplied by the scale" else 1.0)
        m_new = torch.maximum(m, z)
        alpha = torch.exp(m - m_new)
        l = l * alpha + (0.0 if fault == "sink left out of l" else torch.exp(z - m_new))
        m, acc = m_new, acc * alpha
    o = (acc / l).to(BF16)
    lse = m + torch.log(l)
    delta = (do * o.float()).sum(dim=-1, keepdim=True)
    lse_b = m0 + torch.log(l0) if fault == "sink absent from the backward's lse" else lse
    pb = torch.exp(s - lse_b).masked_fill(~allowed, 0.0)
    ds = _bf(pb * (do @ v.mT - delta) * scale)
    out = {"o": o, "lse": lse.squeeze(-1), "dq": ds @ k, "dk": ds.mT @ q, "dv": _bf(pb).mT @ do}
    if z is not None:
        terms = torch.exp(z - lse) * delta
        if fault == "last partial row of dsink dropped":  # FAULT: token t of the batch is summed by workgroup (t / 256) % parts; the last one's row is lost
            parts = max(1, (lse.shape[0] * lse.shape[2] + 255) // 256)
            terms = terms * ((torch.arange(lse.shape[0] * lse.shape[2]).view(lse.shape[0], 1, -1, 1) // 256) % parts != parts - 1)
        out["dsink"] = -terms.sum(dim=(0, 2, 3))
    return out


def _next_row(x, S):
    """[B, H, S, .] -> [B, H, 1, .]: the token row that follows each sample's last in the token-major buffer -- the next sample's first row, and
    for the last sample the NaN rows behind the operand -- or None where the last tile is not ragged."""
    if S % 32 == 0:
        return None
    return torch.cat([x[1:, :, :1], torch.full_like(x[:1, :, :1], float("nan"))], dim=0)


def emulate(c, ops, fault=None):
    """The case through ``_core`` -> the family's tensors as the kernels return them (bf16, fp32 lse / dsink / dk_rope_heads), all [B, H, S, .].
    ``fault``: a key of FAULTS; each changes one expression below or in ``_core``."""
    S = c.S
    al = allowed_of(c)
    ragged = fault == "ragged tile row read as its neighbour"
    if isinstance(c, MlaCase):
        qn, qr, kn, kr, v, do = (t.float() for t in ops)
        H, Dn = c.Hq, c.Dn
        krh = kr[:, None].expand(-1, H, -1, -1)
        if fault == "k_rope not shared":
            krh = torch.stack([kr.roll(-h, dims=1) for h in range(H)], dim=1)  # FAULT: head h reads the rotary key h tokens on
        q, k = torch.cat((qn, qr), dim=-1), torch.cat((kn, krh), dim=-1)
        qs = torch.cat((qn, 0.0 * qr), dim=-1) if fault == "rope half of the score dropped" else None
        r = _core(q, k, v, do, al[:, None], (Dn + c.Dr) ** -0.5, qs=qs, v_next=_next_row(v, S) if ragged else None)
        out = {"o": r["o"], "lse": r["lse"], "dq_nope": r["dq"][..., :Dn].to(BF16), "dq_rope": r["dq"][..., Dn:].to(BF16),
               "dk_nope": r["dk"][..., :Dn].to(BF16), "dk_rope_heads": r["dk"][..., Dn:].clone(), "dv": r["dv"].to(BF16)}
        if fault == "second dK/dV slice at (128, 64) unstored":  # slice 1: dK^T columns 96 .. 191, dV^T columns 64 .. 127; the buffers were NaN
            out["dk_nope"][..., 96:], out["dv"][..., 64:] = float("nan"), float("nan")
            out["dk_rope_heads"][:] = float("nan")
        return out
    if isinstance(c, BandCase):
        q, k, v, do, z = ops
        W = min(c.W, S)
        W = W + 1 if fault == "window one too wide" else W - 1 if fault == "window one too narrow" else W
        al = band_allowed(S, W)
        if fault == "first tile of a row's band dropped":  # FAULT: a row whose band starts in an earlier tile than its own loses that tile
            i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
            first = (i - W + 1).clamp_min(0) // 32
            al = al & ~((j // 32 == first) & (first != i // 32))
        al = al[None].expand(c.B, S, S)
    else:
        q, k, v, do = ops
        z = None
        if fault == "quirk dropped, padded keys masked":
            al = torch.ones(S, S, dtype=torch.bool).tril_()[None] & ga_key_mask(c).bool()[:, None, :]
        if fault == "PLAIN full run as causal":
            al = torch.ones(S, S, dtype=torch.bool).tril_()[None].expand(c.B, S, S)
    rep = c.Hq // c.Hkv
    src = torch.arange(c.Hq) % c.Hkv if fault == "query head mapped to h % Hkv" else torch.arange(c.Hq) // rep
    q, k, v, do = (t.float() for t in (q, k, v, do))
    kx, vx = k[:, src], v[:, src]
    r = _core(q, kx, vx, do, al[:, None], q.shape[-1] ** -0.5, sink=z, fault=fault, v_next=_next_row(vx, S) if ragged else None)
    group = lambda t: t.view(c.B, c.Hkv, rep, S, t.shape[-1]).sum(dim=2).to(BF16)
    out = {"o": r["o"], "lse": r["lse"], "dq": r["dq"].to(BF16), "dk": group(r["dk"]), "dv": group(r["dv"])}
    if "dsink" in r:
        out["dsink"] = r["dsink"]
    if fault == "second dK/dV slice at D = 256 unstored":  # slice 1: columns 128 .. 255 of dk and dv; the buffers were NaN
        out["dk"][..., 128:], out["dv"][..., 128:] = float("nan"), float("nan")
    return out


# ----------------------------------------------------------------------------------------------------------------- the judgement
def _one_key(c, ops):
    """The one-key rules of the case per tensor name, or {} where a sink is a second term of every softmax."""
    if isinstance(c, BandCase) and c.sink in ("rand", "high"):
        return {}
    al = allowed_of(c)
    if isinstance(c, MlaCase):
        qn, qr, kn, kr, v, do = ops
        q, k = torch.cat((qn, qr), dim=-1), torch.cat((kn, kr[:, None].expand(-1, c.Hq, -1, -1)), dim=-1)
        b = one_key_bounds(q, k, v, do, None, False, al)
        out = {"dq_nope": (b["dq"][0], b["dq"][1][..., : c.Dn]), "dq_rope": (b["dq"][0], b["dq"][1][..., c.Dn :])}
        if "dk" in b:
            out.update({"dk_nope": (b["dk"][0], b["dk"][1][..., : c.Dn]), "dk_rope_heads": (b["dk"][0], b["dk"][1][..., c.Dn :])})
        return out
    return one_key_bounds(*ops[:4], None, False, al)


def _sink_terms(c, ops, exact):
    """fp64 pieces of a band case with a sink: p [B, Hq, S, S] (the sink in the denominator), dP = dO V^T, delta [B, Hq, S], w = exp(z - lse)."""
    q, k, v, do, z = ops
    src = torch.arange(c.Hq) // (c.Hq // c.Hkv)
    s = (q.double() @ k.double()[:, src].mT) * c.D ** -0.5
    p = torch.exp(s - exact["lse"].double()[..., None]).masked_fill(~allowed_of(c)[:, None], 0.0)
    dp = do.double() @ v.double()[:, src].mT
    return p, dp, (do.double() * exact["o"].double()).sum(dim=-1), torch.exp(z.double().view(1, -1, 1) - exact["lse"].double())


def dsink_sigma(c, ops, exact):
    """The standard deviation [Hq] of dsink under the kernels' rounding points (module docstring, "Derived bounds" 1)."""
    p, dp, _, w = _sink_terms(c, ops, exact)
    var = ((ops[3].double() * exact["o"].double()) ** 2).sum(dim=-1) + (p ** 2 * dp ** 2).sum(dim=-1)
    return 2.0 ** -8 / 3 ** 0.5 * (w ** 2 * var).sum(dim=(0, 2)).sqrt()


def rounding_variance(x):
    """The variance of one round-to-nearest of x to bf16, element by element: the error is uniform over one ulp = 2^(floor(log2 |x|) - 7)."""
    ulp = torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-300))) - 7)
    return torch.where(x == 0, torch.zeros_like(x), ulp * ulp / 12)


def one_key_sink_sigma(c, ops, exact):
    """{"dq": [B, Hq, blocks], "dk": [B, Hkv, blocks]}: the standard deviation of a block's error norm over the block's norm, for a band case whose
    every softmax is ONE key and a live sink (window of one, or S = 1), else {} (module docstring, "Derived bounds" 2)."""
    if not (isinstance(c, BandCase) and c.sink in ("rand", "high") and min(c.W, c.S) == 1):
        return {}
    q, k, v, do, z = ops
    src = torch.arange(c.Hq) // (c.Hq // c.Hkv)
    p, dp, delta, _ = _sink_terms(c, ops, exact)
    p, dp = p.diagonal(dim1=-2, dim2=-1), dp.diagonal(dim1=-2, dim2=-1)  # [B, Hq, S]: the key's probability and dO . v
    scale = c.D ** -0.5
    t = scale * p * (dp - delta)  # what the kernels round to bf16 as dS
    var_delta = (do.double() ** 2 * rounding_variance(exact["o"].double())).sum(dim=-1)  # of delta = dO . bf16(o)
    u = (scale ** 2 * p ** 2 * var_delta + rounding_variance(t))[..., None]  # variance of the rounded dS of a row, shared by its D elements
    var = {"dq": u * k.double()[:, src] ** 2 + rounding_variance(exact["dq"].double()),
           "dk": (u * q.double() ** 2).view(c.B, c.Hkv, c.Hq // c.Hkv, c.S, c.D).sum(dim=2) + rounding_variance(exact["dk"].double())}
    # _block_norms sums squares: of a square root of the variances it is the variance of the block's error norm
    return {n: (A._block_norms(var[n].sqrt(), c.S) / A._block_norms(exact[n].double(), c.S).clamp_min(1e-300)).sqrt() for n in var}


def one_key_sink_caps(c, ops, exact):
    """The caps of dq and dk in that class: ONE_KEY_SINK_SIGMAS standard deviations, and the plain 8e-3 wherever that is no more."""
    return {n: (ONE_KEY_SINK_SIGMAS * s).clamp_min(GRAD_CAP) for n, s in one_key_sink_sigma(c, ops, exact).items()}


def judge_case(c, got, exact, floor, ops):
    """``got``: the family's tensors [B, H, S, .] on the CPU, lse [B, Hq, S] and (band with a sink) dsink [Hq].
    -> (worst ratio per tensor, lse and dsink, blocks judged, blocks there are, failures)"""
    worst, judged, total, fails = {}, 0, 0, []
    one = _one_key(c, ops)
    caps = one_key_sink_caps(c, ops, exact)
    for name in NAMES[family_of(c)]:
        w, n, f = judge_tensor(name, got[name], exact[name], floor[name], None, one.get(name), caps.get(name, CAP["o"] if name == "o" else GRAD_CAP))
        worst[name] = w
        judged += n
        total += n_blocks(*exact[name].shape[:3])
        fails += f
    lse = got["lse"].double()
    if not bool(torch.isfinite(lse).all()):
        worst["lse"] = math.inf
        fails.append(f"lse: not finite at (sample, head, token) {(~torch.isfinite(lse)).nonzero()[0].tolist()}")
    else:
        d = (lse - exact["lse"].double()).abs()
        worst["lse"] = float(d.max()) / LSE_TOL
        fails += [f"lse: |lse - fp64| = {float(d[b, h, t]):.3e} >= {LSE_TOL:.0e} at sample {b}, head {h}, token {t} (block {min(t // 32, len(block_edges(c.S)) - 1)})"
                  for b, h, t in (d >= LSE_TOL).nonzero().tolist()[:4]]
    if isinstance(c, BandCase) and c.sink is not None:
        dz, ez, fz = got["dsink"].double(), exact["dsink"].double(), floor["dsink"].double()
        sigma = dsink_sigma(c, ops, exact)
        worst["dsink"] = 0.0
        for h in range(c.Hq):
            if not math.isfinite(float(dz[h])):
                worst["dsink"] = math.inf
                fails.append(f"dsink: head {h} not finite")
            elif float(ez[h]) == 0.0:
                if not abs(float(dz[h])) <= DSINK_ZERO_TOL:
                    fails.append(f"dsink: head {h}: exact value is zero, kernel |x| {abs(float(dz[h])):.3e} > {DSINK_ZERO_TOL:.0e}")
                worst["dsink"] = max(worst["dsink"], abs(float(dz[h])) / DSINK_ZERO_TOL)
            else:
                fl = abs(float(fz[h] - ez[h]) / float(ez[h]))
                err = abs(float(dz[h] - ez[h]) / float(ez[h]))
                bound = max(1.5 * fl + (0.0 if fl >= 1e-2 else 2e-3), DSINK_SIGMAS * float(sigma[h] / ez[h].abs()))
                worst["dsink"] = max(worst["dsink"], err / bound)
                if not err <= bound:
                    fails.append(f"dsink: head {h}: {err:.3e} > {bound:.3e} (floor {fl:.3e}, sigma {float(sigma[h] / ez[h].abs()):.3e})")
    return worst, judged, total, fails


def note(tally, c, worst):
    row = tally.setdefault(family_of(c), {})
    for n, w in worst.items():
        row[n] = max(row.get(n, 0.0), w)


def report(label, worst):
    print(f"[side attention sweep] {label}: worst ratio " + "  ".join(f"{n} {w:.3f}" for n, w in worst.items()))


# ----------------------------------------------------------------------------------------------------------------- coverage, derived from a case
BAND_BRANCHES = ("fwd/dQ: kfirst in an earlier 128-block than qb", "fwd/dQ: a wave skips a tile on the window side",
                 "fwd/dQ: a wave skips a tile on the diagonal side", "fwd/dQ: a row's first walked tile holds none of its keys",
                 "fwd/dQ: ragged last key tile", "fwd/dQ: workgroup with fewer than four live waves", "dK/dV: qend set by S",
                 "dK/dV: qend set by the window", "dK/dV: a wave skips a query tile before its keys", "dK/dV: a wave skips a query tile past its window",
                 "dK/dV: rep > 1")
GA_BRANCHES = ("all_keys on", "all_keys off", "NP = 2", "a padded key inside the causal triangle", "a padded key outside the causal triangle")
MLA_BRANCHES = ("NP = 2", "dK^T tiles at columns >= Dn")


def band_branches(c):
    """Which branches of the band kernels the case takes, by walking the loops quoted in the module docstring."""
    S, W = c.S, min(c.W, c.S)  # the host clamps W to S
    t = dict.fromkeys(BAND_BRANCHES, False)
    for qb in range(0, S, 128):
        qlast, kfirst = min(qb + 127, S - 1), max(qb - W + 1, 0)
        t[BAND_BRANCHES[0]] |= kfirst // 128 < qb // 128
        t[BAND_BRANCHES[5]] |= qb + 96 >= S
        for q0 in range(qb, min(qb + 128, S), 32):
            first = True
            for key0 in range(kfirst // 32 * 32, qlast // 32 * 32 + 1, 32):
                if key0 + 31 + W <= q0:
                    t[BAND_BRANCHES[1]] = True
                elif key0 > q0 + 31:
                    t[BAND_BRANCHES[2]] = True
                else:
                    t[BAND_BRANCHES[4]] |= key0 + 31 >= S
                    if first:  # a row whose window starts behind this tile meets online_softmax with m = -inf and a tile of -inf: the m_use path
                        t[BAND_BRANCHES[3]] |= any(max(i - W + 1, 0) > key0 + 31 for i in range(q0, min(q0 + 32, S)))
                    first = False
    for kb in range(0, S, 128):
        klast = min(kb + 127, S - 1)
        qend = min(klast + W - 1, S - 1)
        t[BAND_BRANCHES[6]] |= klast + W - 1 >= S - 1
        t[BAND_BRANCHES[7]] |= klast + W - 1 < S - 1
        for k0 in range(kb, min(kb + 128, S), 32):
            for qs in range(kb // 32 * 32, qend // 32 * 32 + 1, 32):
                t[BAND_BRANCHES[8]] |= qs + 31 < k0
                t[BAND_BRANCHES[9]] |= not qs + 31 < k0 and qs >= k0 + 31 + W
    t[BAND_BRANCHES[10]] = c.Hq // c.Hkv > 1
    return t


def ga_branches(c):
    km = ga_key_mask(c)
    pad = torch.zeros(c.B, c.S, dtype=torch.bool) if km is None else ~km.bool()
    j = torch.arange(c.S)
    all_keys = c.mode == "plain-full" or km is not None
    return {"all_keys on": all_keys, "all_keys off": not all_keys, "NP = 2": c.D == 256,
            "a padded key inside the causal triangle": bool(pad.any()),  # key j <= query j
            "a padded key outside the causal triangle": bool((pad & (j > 0)[None]).any())}  # key j > query 0


def mla_branches(c):
    return {"NP = 2": (c.Dn, c.Dr) == (128, 64), "dK^T tiles at columns >= Dn": True}
