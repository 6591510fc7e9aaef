"""The row kernels of csrc/norm_rope.hip and the SwiGLU / GELU kernels of csrc/elementwise.hip on a real MI355X against fp64 (tests/row_sweep.py): every
dispatch width and its neighbours, the stated maxima, row counts that send a wave round its loop again, every shape of head pass, reduce_rows at the
edges of its unrolled loop -- per row, head or column and element by element, on operands framed in NaN and destinations pre-filled with a bit
pattern; the forwards also against the emulation's rounding points; bit-for-bit structure (row permutations, one-row gradients, repeated launches);
the entries' refusals and the backward wrappers' operand checks.  Every case prints its measured c and its largest error / bound."""

import pytest
import torch

import row_sweep as S

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def tally():
    return {fam: {"judged": 0, "expected": 0, "cases": 0, "c": [], "worst": 0.0} for fam in S.FAMILIES}


def dev(t):
    return S.framed(t, "cuda")


def _settle(fam, case, ex, got, tally, extra=()):
    judged, fails, worst = S.judge(got, ex, case.name)
    S.report(fam, case.name, ex, worst)
    assert ex.c_raw <= S.C_CAP
    fails = fails + list(extra)
    assert not fails, "\n".join(fails)
    assert judged == S.units(ex) == S.expected_units(case), "no row, head or column is left out of the judgement"
    t = tally[fam]
    t["judged"], t["expected"], t["cases"] = t["judged"] + judged, t["expected"] + S.expected_units(case), t["cases"] + 1
    t["c"].append(ex.c)
    t["worst"] = max(t["worst"], worst)


def test_geometry_table_states_the_wrappers_caps(K):
    import os

    if "MI355_NORM_PARTS" not in os.environ:
        assert K.NORM_PARTS == S.NORM_PARTS == S.GEOMETRY["rmsnorm_bwd"]["cap"]
    if "MI355_QK_PARTS" not in os.environ:
        assert K.QK_PARTS == S.QK_PARTS == S.GEOMETRY["qk_bwd"]["cap"]


# ----------------------------------------------------------------------------------------------------------------- launches
def run_rms(K, case, monkeypatch, ns=None):
    ns = S.rms_build(case) if ns is None else ns
    x, w = dev(ns.x), dev(ns.w)
    if case.kind == "fwd":
        y, rstd = K.rmsnorm_fwd(x, w, eps=S.RMS_EPS, want_rstd=case.want_rstd)
        assert (rstd is None) == (not case.want_rstd)
        return {"y": y, "rstd": rstd} if case.want_rstd else {"y": y}
    _, rstd = K.rmsnorm_fwd(x, w, eps=S.RMS_EPS)
    if case.parts:
        monkeypatch.setattr(K, "NORM_PARTS", case.parts)
    dw_out = None
    if case.dw_dtype is not None:
        dw_out = dev(ns.old) if case.dw_acc else S.filled((case.width,), case.dw_dtype, "cuda")
    dx, dw = K.rmsnorm_bwd(x, w, rstd, dev(ns.dy), dev(ns.dres), dw_out=dw_out, dw_accumulate=case.dw_acc)
    assert dw_out is None or dw.data_ptr() == dw_out.data_ptr()
    return {"dx": dx, "dw": dw}


def run_red(K, case):
    from llm_quest_amd import _lib as L

    ns = S.red_build(case)
    part = dev(ns.part)
    dst = dev(ns.old) if case.acc else S.filled((case.n,), case.dtype, "cuda")
    L.require_gpu(part, dst)
    L.call("mi355_reduce_rows_f32", case.parts, case.n, L.ptr(part), L.ptr(dst), L.dt_code(case.dtype), case.acc)
    return {"out": dst}


def run_qk(K, case, monkeypatch, ns=None):
    """-> (outputs, failure strings of the fill checks)"""
    ns = S.qk_build(case) if ns is None else ns
    D, Hq, Hkv, T = case.D, case.Hq, case.Hkv, case.tokens
    qkv, qw, kw, cos, sin, pos = dev(ns.qkv), dev(ns.qw), dev(ns.kw), dev(ns.cos), dev(ns.sin), ns.pos.cuda()
    q, k, rstd = K.qknorm_rope_fwd(qkv, qw, kw, cos, sin, pos, Hq, Hkv, D, eps=S.QK_EPS)
    assert (rstd is None) == (not ns.norm)
    if case.form.startswith("fwd"):
        got = {"y": S.qk_pack(q, k, case)}
        if ns.norm:
            got["rstd"] = rstd
        return got, []
    if case.parts:
        monkeypatch.setattr(K, "QK_PARTS", case.parts)
    dqkv = S.filled(ns.qkv.shape, BF16, "cuda")
    dqw, dkw = K.qknorm_rope_bwd(qkv, qw, kw, cos, sin, pos, rstd, dev(ns.dq), dev(ns.dk), dqkv, Hq, Hkv, D)
    h0 = Hq if ns.konly else 0
    fails = []
    if not S.holds_fill(dqkv[:, (Hq + Hkv) * D :]):
        fails.append(f"{case.name}: the V third of dqkv was written")
    if ns.konly and not S.holds_fill(dqkv[:, : Hq * D]):
        fails.append(f"{case.name}: the query columns of dqkv were written by the key-only form")
    return {"d": dqkv[:, h0 * D : (Hq + Hkv) * D].reshape(T * (Hq + Hkv - h0), D), "dqw": dqw, "dkw": dkw}, fails


def run_ln(K, case, ns=None):
    ns = S.ln_build(case) if ns is None else ns
    x, sc, sh = dev(ns.x), dev(ns.scale), dev(ns.shift)
    if case.kind == "fwd":
        y, mean, rsig = K.layernorm_fwd(x, sc, sh, out_dtype={"f32": F32, "bf16": BF16, "split3": "split3"}[case.out], eps=ns.eps, want_stats=True, mode=case.mode)
        return {"y": y, "mean": mean, "rsig": rsig}
    _, mean, rsig = K.layernorm_fwd(x, sc, sh, out_dtype=F32, eps=ns.eps, want_stats=True, mode=case.mode)
    dsc = S.filled((case.width,), F32, "cuda") if case.dres else None
    dsh = S.filled((case.width,), F32, "cuda") if case.dres else None
    dx, a, b = K.layernorm_bwd(x, sc, mean, rsig, dev(ns.dy), dres=dev(ns.dres), eps=ns.eps, dscale_out=dsc, dshift_out=dsh, mode=case.mode)
    assert dsc is None or (a.data_ptr() == dsc.data_ptr() and b.data_ptr() == dsh.data_ptr())
    return {"dx": dx, "dscale": a, "dshift": b}


def run_act(K, case, ns=None):
    ns = S.act_build(case) if ns is None else ns
    if case.op == "swiglu":
        F = case.F
        gu = dev(ns.gu)
        dgu = K.swiglu_bwd(gu, dev(ns.da), F)
        return {"a": K.swiglu_fwd(gu, F), "du": dgu[:, :F], "dg": dgu[:, F:]}
    x = dev(ns.x.reshape(-1))
    return {"y": K.gelu_fwd(x, tanh=case.kind == 1), "dx": K.gelu_bwd(x, dev(ns.dy.reshape(-1)), tanh=case.kind == 1)}


# ----------------------------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("case", S.rms_fwd_cases() + S.rms_bwd_cases(), ids=lambda c: c.name)
def test_rmsnorm_matches_fp64_per_row_and_column(K, case, tally, monkeypatch):
    got = run_rms(K, case, monkeypatch)
    extra = []
    if case.kind == "fwd":  # against the emulation's rounding points, from the kernel's own rstd (a launch of its own where the case asks for none)
        rstd = got["rstd"] if case.want_rstd else K.rmsnorm_fwd(dev(S.rms_build(case).x), dev(S.rms_build(case).w), eps=S.RMS_EPS)[1]
        extra = S.steps_from(got["y"], S.rms_emulate(case, rstd=rstd)["y"], f"{case.name}: y")
    _settle("rmsnorm", case, S.rms_exact(case), got, tally, extra)


@pytest.mark.parametrize("case", S.red_cases(), ids=lambda c: c.name)
def test_reduce_rows_matches_fp64_per_column(K, case, tally):
    _settle("reduce_rows", case, S.red_exact(case), run_red(K, case), tally)


@pytest.mark.parametrize("case", S.qk_cases(), ids=lambda c: c.name)
def test_qknorm_rope_matches_fp64_per_token_and_head(K, case, tally, monkeypatch):
    got, extra = run_qk(K, case, monkeypatch)
    if case.form.startswith("fwd"):
        extra = extra + S.steps_from(got["y"], S.qk_emulate(case, rstd=got.get("rstd"))["y"], f"{case.name}: y")
    _settle("qknorm_rope", case, S.qk_exact(case), got, tally, extra)


@pytest.mark.parametrize("case", S.ln_fwd_cases() + S.ln_bwd_cases(), ids=lambda c: c.name)
def test_layernorm_matches_fp64_per_row_and_column(K, case, tally):
    got = run_ln(K, case)
    extra = []
    if case.kind == "fwd" and case.out == "split3":
        assert got["y"].shape == (case.rows, 3 * case.width) and got["y"].dtype == BF16
        if not S.ln_split3(got["y"].cpu(), case.width)[1]:
            extra.append(f"{case.name}: the third block of the split3 output is not the first bit for bit")
    _settle("layernorm", case, S.ln_exact(case), S.ln_got(case, got), tally, extra)


@pytest.mark.parametrize("case", S.act_cases(), ids=lambda c: c.name)
def test_swiglu_and_gelu_match_fp64_with_the_special_values(K, case, tally):
    got = run_act(K, case)
    extra = []
    if case.op == "swiglu":
        emu = S.act_emulate(case)
        extra = S.steps_from(got["a"], emu["a"], f"{case.name}: a", floor=S.STEP_FLOOR, alternatives=emu["a_alt"])
    _settle("swiglu_gelu", case, S.act_exact(case), got, tally, extra)


# ----------------------------------------------------------------------------------------------------------------- 2. structure, bit for bit
def _perm(n, seed=5):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed))


def _rows_other_than(t, hot):
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[hot] = False
    return t.detach().cpu()[keep]


def _is_zero(t):
    return bool((t.float() == 0).all())


def _permuted(ns, names, p):
    import copy

    ns2 = copy.copy(ns)
    for name in names:
        if getattr(ns2, name) is not None:
            setattr(ns2, name, getattr(ns2, name)[p].contiguous())
    return ns2


def _assert_same(a, b, what):
    for name in a:
        assert S.same_bits(a[name], b[name]), f"{what}: {name} differs"


@pytest.mark.parametrize("case", [c for c in S.rms_fwd_cases() if c.rows > 8192 and c.width in (520, 1024)], ids=lambda c: c.name)
def test_rmsnorm_forward_commutes_with_a_row_permutation(K, case, monkeypatch):
    ns, p = S.rms_build(case), _perm(case.rows)
    a, b = run_rms(K, case, monkeypatch), run_rms(K, case, monkeypatch, _permuted(S.rms_build(case), ("x",), p))
    assert S.same_bits(a["y"][p.cuda()], b["y"]) and S.same_bits(a["rstd"][p.cuda()], b["rstd"]) and ns.x.shape[0] == case.rows


@pytest.mark.parametrize("case", S.rms_structural_cases(), ids=lambda c: c.name)
def test_rmsnorm_backward_structure(K, case, tally, monkeypatch):
    ns, p = S.rms_build(case), _perm(case.rows)
    a = run_rms(K, case, monkeypatch)
    _assert_same(a, run_rms(K, case, monkeypatch), f"{case.name}: two launches")
    b = run_rms(K, case, monkeypatch, _permuted(ns, ("x", "dy", "dres"), p))
    assert S.same_bits(a["dx"][p.cuda()], b["dx"]), f"{case.name}: dx does not follow the row permutation"
    others = _rows_other_than(a["dx"], case.hot)
    assert S.same_bits(others, _rows_other_than(ns.dres, case.hot)) if case.dres else _is_zero(others), "a row without upstream gradient: dx = dres"
    _settle("rmsnorm", case, S.rms_exact(case), a, tally)


@pytest.mark.parametrize("case", [c for c in S.qk_cases() if c.tokens > 8192] + S.qk_structural_cases(), ids=lambda c: c.name)
def test_qknorm_rope_structure(K, case, tally, monkeypatch):
    ns, p = S.qk_build(case), _perm(case.tokens)
    a, fa = run_qk(K, case, monkeypatch)
    b, fb = run_qk(K, case, monkeypatch, _permuted(ns, ("qkv", "pos", "dq", "dk"), p))
    assert not fa + fb, fa + fb
    T = case.tokens
    main = "y" if case.form.startswith("fwd") else "d"
    per_token = lambda t: t.reshape(T, -1)
    assert S.same_bits(per_token(a[main])[p.cuda()], per_token(b[main])), f"{case.name}: {main} does not follow the token permutation"
    if case.form.startswith("bwd"):
        _assert_same(a, run_qk(K, case, monkeypatch)[0], f"{case.name}: two launches")
        assert _is_zero(_rows_other_than(per_token(a["d"]), case.hot)), "a token without upstream gradient: zero rows"
        _settle("qknorm_rope", case, S.qk_exact(case), a, tally)


@pytest.mark.parametrize("case", [c for c in S.ln_fwd_cases() if c.rows > 8192] + S.ln_structural_cases(), ids=lambda c: c.name)
def test_layernorm_structure(K, case, tally):
    ns, p = S.ln_build(case), _perm(case.rows)
    a, b = run_ln(K, case), run_ln(K, case, _permuted(ns, ("x", "dy", "dres"), p))
    for name in (("y", "mean", "rsig") if case.kind == "fwd" else ("dx",)):
        assert S.same_bits(a[name][p.cuda()], b[name]), f"{case.name}: {name} does not follow the row permutation"
    if case.kind == "bwd":
        _assert_same(a, run_ln(K, case), f"{case.name}: two launches")
        others = _rows_other_than(a["dx"], case.hot)
        assert S.same_bits(others, _rows_other_than(ns.dres, case.hot)) if case.dres else _is_zero(others), "a row without upstream gradient: dx = dres"
        _settle("layernorm", case, S.ln_exact(case), a, tally)


def test_swiglu_commutes_with_a_token_permutation(K):
    case = next(c for c in S.act_cases() if (c.tokens, c.F) == S.SWIGLU_WRAP)
    ns, p = S.act_build(case), _perm(case.tokens)
    a, b = run_act(K, case), run_act(K, case, _permuted(ns, ("gu", "da"), p))
    for name in a:
        assert S.same_bits(a[name][p.cuda()].contiguous(), b[name].contiguous()), name


# ----------------------------------------------------------------------------------------------------------------- 3. refusals
def _refused(name, message, dsts, *args):
    from llm_quest_amd import _lib as L

    L.require_gpu(*dsts)
    with pytest.raises(RuntimeError) as e:
        L.call(name, *[L.ptr(a) if torch.is_tensor(a) or a is None else a for a in args])
    torch.cuda.synchronize()
    assert message in str(e.value), str(e.value)
    assert all(S.holds_fill(d) for d in dsts), f"{name}: a refused call wrote to its destination"


@pytest.mark.parametrize("width", [12, 8200])
def test_rmsnorm_forward_refuses_the_width(K, width):
    x, w = torch.ones(4, width, dtype=BF16, device="cuda"), torch.ones(width, dtype=BF16, device="cuda")
    y, rstd = S.filled((4, width), BF16, "cuda"), S.filled((4,), F32, "cuda")
    _refused("mi355_rmsnorm_fwd", f"mi355_rmsnorm_fwd: width must be a multiple of 8 and <= 8192 (got {width})", (y, rstd), 4, width, x, w, y, rstd, 1e-6)
    with pytest.raises(RuntimeError, match="mi355_rmsnorm_fwd: width must be a multiple of 8"):
        K.rmsnorm_fwd(x, w)


@pytest.mark.parametrize("width", [12, 4104])
def test_rmsnorm_backward_refuses_the_width(K, width):
    x, w, rstd = torch.ones(4, width, dtype=BF16, device="cuda"), torch.ones(width, dtype=BF16, device="cuda"), torch.ones(4, dtype=F32, device="cuda")
    dx, part = S.filled((4, width), BF16, "cuda"), S.filled((1, width), F32, "cuda")
    _refused("mi355_rmsnorm_bwd", f"mi355_rmsnorm_bwd: bad width {width}", (dx, part), 4, width, x, w, rstd, x, None, dx, part, 1)
    with pytest.raises(RuntimeError, match="mi355_rmsnorm_bwd: bad width"):
        K.rmsnorm_bwd(x, w, rstd, x)


def test_layernorm_refuses_the_width(K):
    x, v = torch.ones(4, 6, device="cuda"), torch.ones(6, device="cuda")
    y = S.filled((4, 6), F32, "cuda")
    _refused("mi355_layernorm_fwd", "mi355_layernorm_fwd: width must be a multiple of 4 (got 6)", (y,), 4, 6, x, v, v, y, 1, None, None, 1e-5, 0)
    x, v, st = torch.ones(4, 2052, device="cuda"), torch.ones(2052, device="cuda"), torch.ones(4, device="cuda")
    dx, part = S.filled((4, 2052), F32, "cuda"), S.filled((1, 2 * 2052), F32, "cuda")
    _refused("mi355_layernorm_bwd", "mi355_layernorm_bwd: bad shape (width 2052", (dx, part), 4, 2052, x, v, st, st, x, 1, None, dx, part, 1, 1e-5, 0)
    with pytest.raises(RuntimeError, match="mi355_layernorm_bwd: bad shape"):
        K.layernorm_bwd(x, v, st, st, x)


def test_qknorm_rope_refuses_a_head_dim_of_96(K):
    T, Hq, Hkv, D = 3, 2, 1, 96
    qkv, w = torch.ones(T, (Hq + 2 * Hkv) * D, dtype=BF16, device="cuda"), torch.ones(D, dtype=BF16, device="cuda")
    cs, pos = torch.ones(8, D, device="cuda"), torch.zeros(T, dtype=torch.int32, device="cuda")
    q, k, rstd = S.filled((T, Hq * D), BF16, "cuda"), S.filled((T, Hkv * D), BF16, "cuda"), S.filled((T, Hq + Hkv), F32, "cuda")
    _refused("mi355_qknorm_rope_fwd", "mi355_qknorm_rope_fwd: head_dim must be 64 or 128 (got 96)", (q, k, rstd), T, Hq, Hkv, D, qkv, w, w, cs, cs, pos, q, k, rstd, 1e-6)
    dqkv, part = S.filled(qkv.shape, BF16, "cuda"), S.filled((1, 2 * D), F32, "cuda")
    ones = torch.ones(T, Hq + Hkv, device="cuda")
    dq, dk = torch.ones(T, Hq * D, dtype=BF16, device="cuda"), torch.ones(T, Hkv * D, dtype=BF16, device="cuda")
    _refused("mi355_qknorm_rope_bwd", "mi355_qknorm_rope_bwd: head_dim must be 64 or 128 (got 96)", (dqkv, part), T, Hq, Hkv, D, qkv, w, w, cs, cs, pos, ones, dq, dk, dqkv, part, 1)


def test_swiglu_and_gelu_refuse_a_length_that_is_no_multiple_of_8(K):
    gu, a, dgu = torch.ones(2, 24, dtype=BF16, device="cuda"), S.filled((2, 12), BF16, "cuda"), S.filled((2, 24), BF16, "cuda")
    _refused("mi355_swiglu_fwd", "mi355_swiglu_fwd: F must be a multiple of 8", (a,), 2, 12, gu, a)
    _refused("mi355_swiglu_bwd", "mi355_swiglu_bwd: bad arguments", (dgu,), 2, 12, gu, torch.ones(2, 12, dtype=BF16, device="cuda"), dgu)
    x, y = torch.ones(12, dtype=BF16, device="cuda"), S.filled((12,), BF16, "cuda")
    _refused("mi355_gelu_fwd", "mi355_gelu_fwd: n must be a positive multiple of 8", (y,), 12, x, y, 0)
    _refused("mi355_gelu_bwd", "mi355_gelu_bwd: n must be a positive multiple of 8", (y,), 12, x, x, y, 0)
    with pytest.raises(ValueError, match="gelu_fwd"):
        K.gelu_fwd(x)


# ----------------------------------------------------------------------------------------------------------------- 4. the backward wrappers' operand checks
def test_rmsnorm_bwd_checks_x_w_and_rstd(K):
    x, w = torch.ones(8, 16, dtype=BF16, device="cuda"), torch.ones(16, dtype=BF16, device="cuda")
    rstd, dy = torch.ones(8, device="cuda"), torch.ones(8, 16, dtype=BF16, device="cuda")
    K.rmsnorm_bwd(x, w, rstd, dy)
    xt = torch.ones(16, 8, dtype=BF16, device="cuda").t()
    for bad in ((xt, w, rstd, dy), (x.float(), w, rstd, dy), (x, w.float(), rstd, dy), (x, w[:8], rstd, dy)):
        with pytest.raises(ValueError, match=r"rmsnorm_bwd: x must be contiguous bf16 \[rows,width\], w bf16 \[width\]"):
            K.rmsnorm_bwd(*bad)
    for bad in (rstd.double(), rstd[:4], torch.ones(16, device="cuda")[::2], rstd.to(BF16)):
        with pytest.raises(ValueError, match=r"rmsnorm_bwd: rstd must be contiguous fp32 \[rows\]"):
            K.rmsnorm_bwd(x, w, bad, dy)


def test_swiglu_bwd_checks_gu(K):
    gu, da = torch.ones(8, 32, dtype=BF16, device="cuda"), torch.ones(8, 16, dtype=BF16, device="cuda")
    K.swiglu_bwd(gu, da, 16)
    for bad in (torch.ones(32, 8, dtype=BF16, device="cuda").t(), gu.float(), torch.ones(8, 24, dtype=BF16, device="cuda")):
        with pytest.raises(ValueError, match=r"swiglu_bwd: gu must be contiguous bf16 \[tokens,2F\]"):
            K.swiglu_bwd(bad, da, 16)


def test_gelu_bwd_checks_x(K):
    x = torch.ones(4, 8, dtype=BF16, device="cuda")
    K.gelu_bwd(x, x)
    xt = torch.ones(8, 4, dtype=BF16, device="cuda").t()
    for bad, dy in ((xt, xt), (x.float(), x), (torch.ones(12, dtype=BF16, device="cuda"), torch.ones(12, dtype=BF16, device="cuda"))):
        with pytest.raises(ValueError, match="gelu_bwd: x must be contiguous bf16 with numel % 8 == 0"):
            K.gelu_bwd(bad, dy)


def test_layernorm_bwd_checks_scale_mean_and_rsig(K):
    x, sc, st = torch.randn(8, 16, device="cuda"), torch.ones(16, device="cuda"), torch.ones(8, device="cuda")
    K.layernorm_bwd(x, sc, st, st, x)
    for bad in (sc.to(BF16), sc[:8], torch.ones(32, device="cuda")[::2]):
        with pytest.raises(ValueError, match=r"layernorm_bwd: scale must be contiguous fp32 \[width\]"):
            K.layernorm_bwd(x, bad, st, st, x)
    for bad in (st.double(), st[:4], torch.ones(16, device="cuda")[::2]):
        with pytest.raises(ValueError, match=r"layernorm_bwd: mean must be contiguous fp32 \[rows\]"):
            K.layernorm_bwd(x, sc, bad, st, x)
        with pytest.raises(ValueError, match=r"layernorm_bwd: rsig must be contiguous fp32 \[rows\]"):
            K.layernorm_bwd(x, sc, st, bad, x)


# ----------------------------------------------------------------------------------------------------------------- 5. nothing was left out
def test_zz_every_unit_of_every_case_was_judged(tally):
    n = {fam: len(cases()) for fam, (cases, _, _) in S.FAMILIES.items()}
    if any(tally[f]["cases"] != n[f] for f in n):
        pytest.skip("needs the whole module to have run")
    for fam, t in tally.items():
        print(f"[row sweep] {fam}: {t['cases']} cases, {t['judged']} units judged, c {min(t['c']):.3e} .. {max(t['c']):.3e}, largest error / bound {t['worst']:.3f}")
        assert t["judged"] == t["expected"] == sum(S.expected_units(c) for c in S.FAMILIES[fam][0]())
