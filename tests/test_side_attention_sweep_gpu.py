"""The attention families on the plain 32-key tile layer -- band_* (swa_attn_*, sink_attn_*), ga_* (attn_generic_*, attn_dropout_* at p = 0) and mla_* --
against fp64 on a real MI355X, block by block (tests/side_attention_sweep.py): lengths and windows on and next to every 32- and 128-token edge,
every built head-dim pair, GQA ratios 1 to 6, sinks (random, far below, far above), the quirk and PLAIN masks, packed and column-sliced operands.
Every caller-provided output is pre-filled with NaN (dq, dk, dv everywhere; o, dq_rope and dk_rope_heads of mla), every operand has 32 rows of NaN
behind its last token, and whatever surrounds a destination must come back untouched.  NOT pre-filled: o and lse of the band and ga families and lse
of mla, which their wrappers allocate themselves (torch.empty, no out= parameter): a forward row that is never stored would show there only as
stale allocator contents judged against fp64.  Every case prints its worst ratio (kernel / bound) per tensor; the last test prints the worst per family."""

import pytest
import torch

import side_attention_sweep as X
from attention_sweep import from_tokens, to_tokens

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
MARGIN = 8  # columns on either side of a sliced operand: 16 bytes, so the slice stays 16-byte aligned and the pitch a multiple of 8
GUARD = 7.0  # what surrounds a destination


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from types import SimpleNamespace

    from llm_quest_amd import kernels, kernels_g3, kernels_mimo, kernels_mla, kernels_q35

    return SimpleNamespace(K=kernels, G3=kernels_g3, MIMO=kernels_mimo, MLA=kernels_mla, Q35=kernels_q35)


@pytest.fixture(scope="module")
def tally():
    return {}


def _src(x4, margin):
    """[B, H, S, D] on the CPU -> the token-major [B*S, H*D] device view the kernels read: NaN rows behind the last token and, with a margin, NaN
    columns on either side (a column slice of a wider buffer)."""
    t = to_tokens(x4)
    buf = torch.full((t.shape[0] + X.TAIL_ROWS, t.shape[1] + 2 * margin), float("nan"), dtype=BF16, device="cuda")
    view = buf[: t.shape[0], margin : margin + t.shape[1]]
    view.copy_(t)
    return view


def _src_rows(x2, margin):
    return _src(x2[:, None], margin)  # [B, S, D]: one "head"


class _Dest:
    """A destination [rows, width] pre-filled with NaN inside a buffer of GUARD: ``check`` asserts that the guard rows and columns are untouched."""

    def __init__(self, rows, width, margin, dtype=BF16):
        self.buf = torch.full((rows + X.TAIL_ROWS, width + 2 * margin), GUARD, dtype=dtype, device="cuda")
        self.view = self.buf[:rows, margin : margin + width]
        self.view.fill_(float("nan"))
        self.rows, self.margin, self.width = rows, margin, width

    def check(self, name):
        b, m = self.buf, self.margin
        assert bool((b[self.rows :] == GUARD).all()) and bool((b[:, :m] == GUARD).all()) and bool((b[:, m + self.width :] == GUARD).all()), \
            f"{name}: the rows and columns around the destination are untouched"


def _run_band(M, c, ops, margin=0):
    """-> (tensors [B, H, S, .] on the CPU for the judgement, the raw device outputs for bit comparisons)"""
    q, k, v, do, z = ops
    B, S, Hq, Hkv, D, DV, T = c.B, c.S, c.Hq, c.Hkv, c.D, c.DV, c.B * c.S
    qd, kd, vd, dod = (_src(t, margin) for t in (q, k, v, do))
    dq, dk, dv = _Dest(T, Hq * D, margin), _Dest(T, Hkv * D, margin), _Dest(T, Hkv * DV, margin)
    if c.entry == "swa":
        o, lse = M.G3.swa_attn_fwd(qd, kd, vd, B, S, Hq, Hkv, D, c.W)
        M.G3.swa_attn_bwd(qd, kd, vd, o, dod, lse, B, S, Hq, Hkv, D, c.W, dq.view, dk.view, dv.view)
        dz = None
    else:
        zd = None if z is None else z.cuda()
        o, lse = M.MIMO.sink_attn_fwd(qd, kd, vd, B, S, Hq, Hkv, D, DV, c.W, sink=zd)
        dz = M.MIMO.sink_attn_bwd(qd, kd, vd, o, dod, lse, B, S, Hq, Hkv, D, DV, c.W, sink=zd, dq=dq.view, dk=dk.view, dv=dv.view)[3]
    torch.cuda.synchronize()
    for n, d in (("dq", dq), ("dk", dk), ("dv", dv)):
        d.check(n)
    raw = {"o": o, "lse": lse, "dq": dq.view, "dk": dk.view, "dv": dv.view}
    got = {"o": from_tokens(o.cpu(), B, S, Hq, DV), "lse": lse.cpu(), "dq": from_tokens(dq.view.cpu(), B, S, Hq, D),
           "dk": from_tokens(dk.view.cpu(), B, S, Hkv, D), "dv": from_tokens(dv.view.cpu(), B, S, Hkv, DV)}
    if c.sink is not None:
        raw["dsink"] = dz
        got["dsink"] = dz.cpu()
    else:
        assert dz is None
    return got, raw


def _run_ga(M, c, ops, margin=0):
    B, S, Hq, Hkv, D, T = c.B, c.S, c.Hq, c.Hkv, c.D, c.B * c.S
    qd, kd, vd, dod = (_src(t, margin) for t in ops)
    dq, dk, dv = _Dest(T, Hq * D, margin), _Dest(T, Hkv * D, margin), _Dest(T, Hkv * D, margin)
    if c.mode.startswith("plain"):  # the PLAIN semantics: the dropout entry points at p = 0
        causal = c.mode == "plain-causal"
        o, lse = M.K.attn_dropout_fwd(qd, kd, vd, B, S, Hq, Hkv, D, 0.0, 1234, 0, causal=causal)
        M.K.attn_dropout_bwd(qd, kd, vd, o, dod, lse, B, S, Hq, Hkv, D, dq.view, dk.view, dv.view, 0.0, 1234, 0, causal=causal)
    else:
        km = X.ga_key_mask(c)
        kmd = None if km is None else km.cuda()
        o, lse = M.Q35.attn_generic_fwd(qd, kd, vd, B, S, Hq, Hkv, D, key_mask=kmd)
        M.Q35.attn_generic_bwd(qd, kd, vd, o, dod, lse, B, S, Hq, Hkv, D, dq.view, dk.view, dv.view, key_mask=kmd)
    torch.cuda.synchronize()
    for n, d in (("dq", dq), ("dk", dk), ("dv", dv)):
        d.check(n)
    raw = {"o": o, "lse": lse, "dq": dq.view, "dk": dk.view, "dv": dv.view}
    got = {"o": from_tokens(o.cpu(), B, S, Hq, D), "lse": lse.cpu(), "dq": from_tokens(dq.view.cpu(), B, S, Hq, D),
           "dk": from_tokens(dk.view.cpu(), B, S, Hkv, D), "dv": from_tokens(dv.view.cpu(), B, S, Hkv, D)}
    return got, raw


def _run_mla(M, c, ops, margin=0):
    qn, qr, kn, kr, v, do = ops
    B, S, H, Dn, Dr, T = c.B, c.S, c.Hq, c.Dn, c.Dr, c.B * c.S
    qnd, qrd, knd, vd, dod = (_src(t, margin) for t in (qn, qr, kn, v, do))
    krd = _src_rows(kr, margin)
    o, dqn, dqr, dkn, dv = _Dest(T, H * Dn, margin), _Dest(T, H * Dn, margin), _Dest(T, H * Dr, margin), _Dest(T, H * Dn, margin), _Dest(T, H * Dn, margin)
    dkr = _Dest(T, H * Dr, 0, F32)  # the per-head scratch is contiguous by contract
    _, lse = M.MLA.mla_attn_fwd(qnd, qrd, knd, krd, vd, B, S, H, Dn, Dr, o=o.view)
    M.MLA.mla_attn_bwd(qnd, qrd, knd, krd, vd, o.view, dod, lse, B, S, H, Dn, Dr, dq_nope=dqn.view, dq_rope=dqr.view, dk_nope=dkn.view, dv=dv.view,
                       dk_rope_heads=dkr.view.view(T, H, Dr))
    torch.cuda.synchronize()
    dests = {"o": o, "dq_nope": dqn, "dq_rope": dqr, "dk_nope": dkn, "dk_rope_heads": dkr, "dv": dv}
    for n, d in dests.items():
        d.check(n)
    raw = {n: d.view for n, d in dests.items()}
    raw["lse"] = lse
    got = {n: from_tokens(d.view.cpu(), B, S, H, d.width // H) for n, d in dests.items()}
    got["lse"] = lse.cpu()
    return got, raw


RUN = {"band": _run_band, "ga": _run_ga, "mla": _run_mla}
OPERANDS = {"band": X.band_operands, "ga": X.ga_operands, "mla": X.mla_operands}


def _case(M, c, tally):
    fam = X.family_of(c)
    ops = OPERANDS[fam](c)
    exact, floor = X.reference(c, ops)
    got, _ = RUN[fam](M, c, ops, MARGIN if fam == "mla" and c.sliced else 0)
    worst, judged, total, fails = X.judge_case(c, got, exact, floor, ops)
    X.report(f"{fam} {X.case_id(c)}", worst)
    assert not fails, X.case_id(c) + "\n" + "\n".join(fails)
    assert judged == total == X.blocks_of(c), "no block is left out of the judgement"
    X.note(tally, c, worst)


@pytest.mark.parametrize("case", X.band_cases(), ids=X.case_id)
def test_band_attention_matches_fp64_block_by_block(M, case, tally):
    _case(M, case, tally)


@pytest.mark.parametrize("case", X.ga_cases(), ids=X.case_id)
def test_generic_attention_matches_fp64_block_by_block(M, case, tally):
    _case(M, case, tally)


@pytest.mark.parametrize("case", X.mla_cases(), ids=X.case_id)
def test_mla_attention_matches_fp64_block_by_block(M, case, tally):
    _case(M, case, tally)


# ----------------------------------------------------------------------------------------------------------------- column slices of wider buffers
def _first(cases, pred):
    return next(c for c in cases if pred(c))


STRIDED = [
    _first(X.band_cases(), lambda c: c.S == 129 and c.sink == "rand" and c.W < c.S),
    _first(X.band_cases(), lambda c: c.S == 65 and c.entry == "swa" and c.Hq > c.Hkv),
    _first(X.ga_cases(), lambda c: c.S == 129 and c.D == 256),
    _first(X.ga_cases(), lambda c: 33 <= c.S <= 129 and c.mode == "plain-full"),
    _first(X.mla_cases(), lambda c: c.S == 129 and (c.Dn, c.Dr) == (128, 64)),
    _first(X.mla_cases(), lambda c: c.S == 65 and (c.Dn, c.Dr) == (64, 32)),
]


@pytest.mark.parametrize("case", STRIDED, ids=lambda c: X.family_of(c) + "-" + X.case_id(c))
def test_column_slices_of_wider_buffers_give_the_packed_bits(M, case):
    """q, k, v, dO and every caller-provided destination as column slices (row pitch = the packed width plus a margin on both sides): the packed
    run's bits, and the margins untouched (``_Dest.check`` inside the run)."""
    fam = X.family_of(case)
    ops = OPERANDS[fam](case)
    _, packed = RUN[fam](M, case, ops, 0)
    _, sliced = RUN[fam](M, case, ops, MARGIN)
    assert packed.keys() == sliced.keys()
    for name in packed:
        assert bool(torch.isfinite(packed[name].float()).all()), name
        assert torch.equal(packed[name], sliced[name]), name


def test_zz_worst_ratio_per_family(tally):
    """Runs after the tables: the GPU column of side_attention_sweep.MEASURED and of DESIGN.md section 4."""
    if set(tally) != {"band", "ga", "mla"}:
        pytest.skip("needs the three tables to have run")
    for fam, row in tally.items():
        X.report(f"MI355X, {fam}, all cases", row)
    for fam, row in tally.items():
        assert max(row.values()) <= 1.0, (fam, row)
