"""The judgement of the row-kernel sweep (tests/row_sweep.py) is sound: per family an fp32 emulation of the kernels' order of operations passes it in
every case with every unit judged, the measured c stays under its cap, the cases cover what they claim to cover (asserted from the geometry table),
and a defect planted in the emulation is named by case and row, head or column.  Runs without a GPU; prints the measured c range per family."""

import re

import pytest
import torch

import row_sweep as S

BF16, F32 = torch.bfloat16, torch.float32
ALL = [(fam, case) for fam, (cases, _, _) in S.FAMILIES.items() for case in cases()]


@pytest.fixture(scope="module")
def tally():
    return {fam: {"c_raw": [], "c": [], "judged": 0, "cases": 0, "worst": 0.0} for fam in S.FAMILIES}


@pytest.mark.parametrize("fam,case", ALL, ids=lambda v: v if isinstance(v, str) else v.name)
def test_emulation_is_inside_the_bound_with_everything_judged(fam, case, tally):
    _, exact, emulate = S.FAMILIES[fam]
    ex = exact(case)
    judged, fails, worst = S.judge(emulate(case), ex, case.name)
    S.report(fam, case.name, ex, worst)
    assert ex.c_raw <= S.C_CAP, f"{case.name}: the fp32 reference alone needs c = {ex.c_raw:.3e} > 2^-10: wrong inputs for this test"
    assert S.C_FLOOR <= ex.c <= S.C_CAP
    assert not fails, "\n".join(fails)
    assert judged == S.units(ex) == S.expected_units(case), "no row, head or column is left out of the judgement"
    t = tally[fam]
    t["c_raw"].append(ex.c_raw), t["c"].append(ex.c)
    t["judged"], t["cases"], t["worst"] = t["judged"] + judged, t["cases"] + 1, max(t["worst"], worst)


def test_zz_range_of_c_per_family(tally):
    if sum(t["cases"] for t in tally.values()) != len(ALL):
        pytest.skip("needs the whole module to have run")
    for fam, t in tally.items():
        print(f"[row sweep] {fam}: {t['cases']} cases, {t['judged']} units, 64 x fp32 reference error {min(t['c_raw']):.3e} .. {max(t['c_raw']):.3e}, "
              f"c {min(t['c']):.3e} .. {max(t['c']):.3e}, emulation's largest error / bound {t['worst']:.3f}")
        assert max(t["c"]) <= S.C_CAP


# ----------------------------------------------------------------------------------------------------------------- operands
def test_operands_are_framed_in_nan_aligned_and_hold_the_special_rows():
    x = torch.arange(24, dtype=F32).view(3, 8)
    for t in (x, x.to(BF16)):
        v = S.framed(t)
        store = v.untyped_storage()
        whole = torch.empty(0, dtype=t.dtype).set_(store)
        assert whole.numel() == t.numel() + 2 * S.PAD and v.storage_offset() == S.PAD and (v.storage_offset() * t.element_size()) % 16 == 0
        assert v.is_contiguous() and torch.equal(v, t) and int(torch.isfinite(whole.float()).sum()) == t.numel(), "everything around the operand is NaN"
    for dt in (BF16, F32):
        f = S.filled((3, 5), dt)
        assert S.holds_fill(f) and bool((f.float() != 0).all()) and bool(torch.isfinite(f.float()).all())
        f[1, 2] = 0
        assert not S.holds_fill(f)
    ns = S.rms_build(S.rms_bwd_cases()[2])  # 50 rows
    assert float(ns.x[1].float().abs().max()) == 0 and float(ns.x[0].float().abs().max()) > 64 and float(ns.x[-1].float().abs().max()) < 0.2
    ln = S.ln_build(S.ln_fwd_cases()[0])
    assert all(float(r.std()) > 0 for r in ln.x), "no constant row for LayerNorm"
    for case in S.qk_cases():
        pos = S.qk_positions(case.tokens).tolist()
        assert 0 <= min(pos) and max(pos) == S.QK_CTX - 1 and (case.tokens < 2 or 0 in pos)
        if case.tokens >= 5:
            assert len(set(pos)) < len(pos) and pos != sorted(pos), "repeats, not monotonic"
    qk = S.qk_build(S.qk_cases()[0])
    assert not torch.equal(qk.cos[:, : qk.cos.shape[1] // 2], qk.cos[:, qk.cos.shape[1] // 2 :]), "the table's halves differ: a half mix-up shows"


def test_special_values_sit_in_the_gate_and_the_reference_is_finite_there():
    for case in S.act_cases():
        ns, ex = S.act_build(case), S.act_exact(case)
        grid = ns.gu[:, case.F :] if case.op == "swiglu" else ns.x
        held = min(len(S.SPECIALS), grid.numel())
        assert held == len(S.SPECIALS) or case.n == 8
        rows = grid.shape[0]
        for i, v in enumerate(S.SPECIALS[:held]):
            got = float(grid[i % rows, i // rows])
            assert got == v and (v != 0 or str(got) == str(v)), (case.name, v)
        assert all(bool(torch.isfinite(o.ref).all()) for o in ex.outs.values())
    # sigmoid goes through exp overflow at the +-89 pair: fp32 exp(89) is inf, and the fp32 evaluation underflows where fp64 does not
    assert torch.exp(torch.tensor(89.0)).isinf() and float(torch.sigmoid(torch.tensor(-89.0))) == 0 < float(torch.sigmoid(torch.tensor(-89.0, dtype=torch.float64)))


# ----------------------------------------------------------------------------------------------------------------- coverage, from the geometry table
def test_rmsnorm_cases_cover_row_loops_lanes_and_dispatch():
    fwd, bwd = S.rms_fwd_cases(), S.rms_bwd_cases()
    assert {c.width for c in fwd} == set(S.RMS_FWD_WIDTHS) and {c.width for c in bwd} == set(S.RMS_BWD_WIDTHS)
    assert S.first_wrap("rmsnorm_fwd") == 8195 and S.RMS_WRAP_BWD == 2053
    for c in fwd:
        wrap = c.rows == 8195
        assert (S.trips("rmsnorm_fwd", c.rows) == 2) == wrap and S.last_trip_partial("rmsnorm_fwd", c.rows) == wrap
        assert S.trips("rmsnorm_fwd", c.rows - 3 if wrap else c.rows) == 1, "8192 rows are one trip; 8195 give three waves a second row and leave the last trip partial"
    assert {c.width for c in fwd if c.rows == 8195} == {8, 520, 1024}
    assert {S.branch("rmsnorm_fwd", w) for w in S.RMS_FWD_WIDTHS} == {"generic", "rowreg2"} and S.branch("rmsnorm_fwd", 1024) == "rowreg2"
    assert all(S.branch("rmsnorm_fwd", w) == "generic" for w in (1016, 1032, 512))
    assert {S.branch("rmsnorm_fwd", c.width) for c in fwd if not c.want_rstd} == {"generic", "rowreg2"}
    assert max(S.RMS_FWD_WIDTHS) == S.GEOMETRY["rmsnorm_fwd"]["max_width"] and max(S.RMS_BWD_WIDTHS) == S.GEOMETRY["rmsnorm_bwd"]["max_width"]
    assert S.GEOMETRY["rmsnorm_bwd"]["lds_bytes_per_col"] * 4096 == 65536
    assert {w: S.branch("rmsnorm_bwd", w) for w in (504, 512, 520, 1016, 1024, 1032)} == {504: "generic", 512: "rowreg1", 520: "generic", 1016: "generic", 1024: "rowreg2", 1032: "generic"}
    generic = [w for w in S.RMS_BWD_WIDTHS if S.branch("rmsnorm_bwd", w) == "generic"]
    assert {S.lane_vectors("rmsnorm_bwd", w) for w in generic} >= {1, 2, 8}, "idle lanes, a second vector, the maximum"
    assert S.lane_vectors("rmsnorm_fwd", 504) == 1 and S.lane_vectors("rmsnorm_fwd", 520) == 2 and S.lane_vectors("rmsnorm_fwd", 8192) == 16
    for w in S.RMS_BWD_WIDTHS:
        mine = [c for c in bwd if c.width == w]
        assert {c.dres for c in mine} == {False, True}
        small = [c for c in mine if c.parts == 3]
        assert len(small) == 1 and small[0].rows == 50
        assert S.trips("rmsnorm_bwd", 50, 3) == 5 and 50 // (4 * 3) == 4 and S.last_trip_partial("rmsnorm_bwd", 50, 3), "every wave walks four or five rows"
    assert {c.width for c in bwd if c.rows == 2053} == {512, 520, 1024}
    assert S.trips("rmsnorm_bwd", 2053) == 2 and S.last_trip_partial("rmsnorm_bwd", 2053) and S.trips("rmsnorm_bwd", 2048) == 1
    for kernel in ("rowreg1", "generic", "rowreg2"):
        assert {(c.dw_dtype, c.dw_acc) for c in bwd if c.dw_dtype is not None and S.branch("rmsnorm_bwd", c.width) == kernel} == {(BF16, False), (BF16, True), (F32, False), (F32, True)}
    assert all(S.trips("rmsnorm_bwd", c.rows) == 2 and 0 < c.hot < c.rows for c in S.rms_structural_cases())


def test_reduce_rows_cases_cover_the_unrolled_loop_and_its_tail():
    cases = S.red_cases()
    assert {c.parts for c in cases} == set(S.RED_PARTS) and {c.n for c in cases} == set(S.RED_N)
    for p in S.RED_PARTS:
        assert {(c.dtype, c.acc) for c in cases if c.parts == p} == {(F32, 0), (F32, 1), (BF16, 0), (BF16, 1)}
    walk = {p: [S.reduce_walk(p, lane) for lane in range(16)] for p in S.RED_PARTS}
    assert walk[48] == [(0, 3)] * 16 and walk[49] == [(1, 0)] + [(0, 3)] * 15, "48: tail only; 49: the first lane's first unrolled trip"
    assert walk[64] == [(1, 0)] * 16 and walk[65] == [(1, 1)] + [(1, 0)] * 15, "64: unrolled, no tail; 65: unrolled and a tail"
    assert walk[113][0] == (2, 0) and walk[113][1] == (1, 3) and walk[512] == [(8, 0)] * 16
    assert walk[1][1] == (0, 0) and walk[15][15] == (0, 0) and walk[17][0] == (0, 2), "idle part-lanes"
    assert all(sum(u * 4 + t for u, t in w) == p for p, w in walk.items()), "every part is read once"
    assert {n % 64 for n in S.RED_N} >= {0, 1, 63}, "full, ragged and single-column blocks"


def test_qk_head_sets_cover_the_passes():
    cases = S.qk_cases()
    for D in (64, 128):
        hpw = S.GEOMETRY["qk_fwd"]["HPW"][D]
        assert hpw == 64 // (D // 16)
        sets = {(c.Hq, c.Hkv) for c in cases if c.D == D}
        assert sets >= set(S.QK_HEADS)
        passes = {hs: S.head_passes(D, *hs) for hs in sets}
        assert any(len(p) == 1 and None not in p[0] for p in passes.values()), "a full single pass"
        assert any(len(p) == 1 and None in p[0] for p in passes.values()), "one pass with idle slots"
        assert any("q" in one and "k" in one for p in passes.values() for one in p[1:]), "a later pass that straddles the q/k boundary"
        assert any(len(p) > 1 and sum(s is not None for s in p[-1]) == 1 for p in passes.values()), "a last pass with one valid slot"
        assert any(len(p) == 3 for p in passes.values()), "three passes"
        assert any(len(S.head_passes(D, *hs, konly=True)) > 1 for hs in sets if any(c.form == "bwd_k" and (c.Hq, c.Hkv) == hs and c.D == D for c in cases)), "key-only, more than one pass"
        for hs in S.QK_HEADS:
            assert {c.form for c in cases if c.D == D and (c.Hq, c.Hkv) == hs} == set(S.QK_FORMS)
        assert {c.tokens for c in cases if c.D == D and c.parts is None and c.tokens < 10} == set(S.QK_TOKENS)
        small = [c for c in cases if c.D == D and c.parts == 2]
        assert small and all(c.tokens == 21 and S.qk_parts(21, c.Hq, c.Hkv, D, 2) == 2 for c in small)
        assert S.trips("qk_bwd", 21, 2) == 3 and S.last_trip_partial("qk_bwd", 21, 2)
        big = [c for c in cases if c.D == D and c.tokens == S.QK_WRAP_BWD]
        assert {c.form for c in big} == {"bwd", "bwd_k"} and all((c.Hq, c.Hkv) == (4, 2) and S.qk_parts(c.tokens, 4, 2, D) == S.QK_PARTS for c in big)
    assert S.QK_WRAP_BWD == 3077 and S.trips("qk_bwd", 3077) == 2 and S.last_trip_partial("qk_bwd", 3077) and S.trips("qk_bwd", 3072) == 1
    wrap = [c for c in cases if c.form == "fwd" and c.tokens == 8195]
    assert [(c.D, c.Hq, c.Hkv) for c in wrap] == [(64, 1, 1)] and S.trips("qk_fwd", 8195) == 2


def test_layernorm_cases_cover_row_loops_lanes_and_dispatch():
    fwd, bwd = S.ln_fwd_cases(), S.ln_bwd_cases()
    for w in S.LN_WIDTHS:
        assert {(c.mode, c.out) for c in fwd if c.width == w and c.rows < 10} == {(m, o) for m in (0, 1) for o in S.LN_OUTS}
        assert {(c.mode, c.dy_bf16, c.dres) for c in bwd if c.width == w and c.rows < 10} == {(m, b, r) for m in (0, 1) for b in (False, True) for r in (False, True)}
    assert {c.rows for c in fwd if c.rows < 10} == {c.rows for c in bwd if c.rows < 10} == set(S.LN_ROWS)
    for kernel in ("layernorm_fwd", "layernorm_bwd"):
        assert {w: S.branch(kernel, w) for w in (764, 768, 772, 1024, 1028)} == {764: "generic", 768: "rowreg3", 772: "generic", 1024: "rowreg4", 1028: "generic"}
        assert S.lane_vectors(kernel, 252) == 1 and S.lane_vectors(kernel, 256) == 1 and S.lane_vectors(kernel, 260) == 2 and S.lane_vectors(kernel, 2048) == 8
    assert max(S.LN_WIDTHS) == S.GEOMETRY["layernorm_bwd"]["max_width"] and S.GEOMETRY["layernorm_bwd"]["lds_bytes_per_col"] * 2048 == 65536
    assert {c.width for c in fwd if c.rows == 8195} == {192, 768} and S.trips("layernorm_fwd", 8195) == 2 and S.trips("layernorm_fwd", 8192) == 1
    assert {c.width for c in bwd if c.rows == 4101} == {192, 768} and S.LN_WRAP_BWD == 4101
    assert S.trips("layernorm_bwd", 4101) == 2 and S.last_trip_partial("layernorm_bwd", 4101) and S.trips("layernorm_bwd", 4096) == 1
    assert {S.branch("layernorm_bwd", c.width) for c in S.ln_structural_cases()} == {"generic", "rowreg3"}


def test_element_cases_cover_the_second_trip():
    cases = S.act_cases()
    assert S.ONE_TRIP == 524288
    sw = {(c.tokens, c.F): S.element_trips("swiglu", c.tokens * c.F // 8) for c in cases if c.op == "swiglu"}
    assert {F for _, F in sw} == {8, 72, 3072, 3080} and {t for t, _ in sw} == {1, 3, 5, 1366}
    assert sw.pop(S.SWIGLU_WRAP) == 2 and set(sw.values()) == {1} and 1366 * 3080 // 8 == 525910
    for kind in (0, 1):
        ge = {c.n: S.element_trips("gelu", c.n // 8) for c in cases if c.op == "gelu" and c.kind == kind}
        assert ge == {8: 1, 8 * 257: 1, 8 * (524288 + 257): 2}


def test_layernorm_closed_form_equals_fp64_autograd():
    for case in S.ln_bwd_cases()[:16] + S.ln_bwd_cases()[40:48]:
        ex, (dx, dsc, dsh) = S.ln_exact(case), S.ln_autograd(case)
        for name, want in (("dx", dx), ("dscale", dsc), ("dshift", dsh)):
            ref = ex.outs[name].ref
            assert float((ref - want.reshape(ref.shape)).abs().max()) <= 1e-11 * float(ex.outs[name].mag.max()), (case.name, name)


# ----------------------------------------------------------------------------------------------------------------- planted defects
def _case(cases, name):
    return next(c for c in cases if c.name == name)


def _named_units(fails, case, output):
    assert fails, f"{case.name}: the planted defect was not found"
    units = []
    for f in fails:
        assert f.startswith(case.name + ": ")
        m = re.match(rf"{re.escape(case.name)}: {output}, [a-z(), ]+ (\d+)", f)
        if m:
            units.append(int(m.group(1)))
    assert units, f"{case.name}: no failure names output {output}: {fails}"
    return units


def test_a_waves_missing_last_trip_is_named_by_column():
    case = _case(S.rms_bwd_cases(), "rms-bwd-50x520-dres-parts3")
    _, fails, _ = S.judge(S.rms_emulate(case, "drop_last_trip"), S.rms_exact(case), case.name)
    assert all(0 <= u < 520 for u in _named_units(fails, case, "dw")) and all(": dw, column " in f for f in fails), fails


def test_a_mean_over_the_padded_vector_count_is_named_by_row():
    case = next(c for c in S.rms_fwd_cases() if c.width == 504)
    assert S.lane_vectors("rmsnorm_fwd", 504) * 64 * 8 == 512 != 504
    _, fails, _ = S.judge(S.rms_emulate(case, "mean_over_padded_vectors"), S.rms_exact(case), case.name)
    assert set(_named_units(fails, case, "rstd")) <= set(range(case.rows)) and any(": rstd, row " in f for f in fails), fails
    same = next(c for c in S.rms_fwd_cases() if c.width == 512)
    assert not S.judge(S.rms_emulate(same, "mean_over_padded_vectors"), S.rms_exact(same), same.name)[1], "at 512 the padded count is the width"


def test_key_heads_normalised_with_the_query_weight_are_named_by_head():
    case = next(c for c in S.qk_cases() if c.form == "fwd" and (c.Hq, c.Hkv, c.D) == (4, 2, 128))
    _, fails, _ = S.judge(S.qk_emulate(case, "key_heads_with_query_weight"), S.qk_exact(case), case.name)
    assert all(u % 6 >= 4 for u in _named_units(fails, case, "y")), fails


def test_an_unwritten_second_head_pass_is_named_by_head():
    case = next(c for c in S.qk_cases() if c.form == "fwd" and (c.Hq, c.Hkv, c.D) == (16, 8, 128))
    _, fails, _ = S.judge(S.qk_emulate(case, "second_pass_unwritten"), S.qk_exact(case), case.name)
    assert all(8 <= u % 24 < 16 for u in _named_units(fails, case, "y")), fails


def test_swapped_layernorm_modes_are_named_by_row():
    for mode in (0, 1):
        case = next(c for c in S.ln_fwd_cases() if c.mode == mode and c.out == "f32" and c.rows == 5 and c.width >= 192)
        _, fails, _ = S.judge(S.ln_got(case, S.ln_emulate(case, "modes_swapped")), S.ln_exact(case), case.name)
        assert 4 in _named_units(fails, case, "rsig"), f"the row scaled by 2^-6 is where the modes differ most: {fails}"


def test_a_dropped_reduce_rows_tail_is_named_by_column():
    case = next(c for c in S.red_cases() if c.parts == 49 and c.dtype == F32 and not c.acc)
    _, fails, _ = S.judge(S.red_emulate(case, "drop_tail"), S.red_exact(case), case.name)
    assert all(0 <= u < case.n for u in _named_units(fails, case, "out")) and all("column" in f for f in fails)


def test_exchanged_swiglu_halves_are_named_by_token():
    case = _case(S.act_cases(), "swiglu-3x3072")
    _, fails, _ = S.judge(S.act_emulate(case, "halves_exchanged"), S.act_exact(case), case.name)
    assert set(_named_units(fails, case, "a")) <= {0, 1, 2} and any(": a, token " in f for f in fails), fails


def test_a_nan_or_inf_is_named():
    case = next(c for c in S.rms_fwd_cases() if c.width == 504)
    got = S.rms_emulate(case)
    got["y"][3, 17] = float("inf")
    judged, fails, _ = S.judge(got, S.rms_exact(case), case.name)
    assert fails == [f"{case.name}: y, row 3: not finite at element 17"] and judged == S.expected_units(case)


def test_a_sigmoid_off_in_its_last_bits_passes_the_step_criterion_at_each_rounding_point():
    """What a hardware exp and reciprocal do to SwiGLU: the fp32 sigmoid one part in 2^22 up or down.  Measured against the plain emulation alone the
    forward is then now and then two steps away (printed); measured at each rounding point it is never more than one."""
    t = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.0e38, 2.0 ** -126]).to(BF16)
    assert S.bf16_step(t, 1).float().tolist()[:2] == [1.0078125, -1.0078125] and S.bf16_step(t, -1).float().tolist()[:2] == [0.99609375, -0.99609375]
    assert S.bf16_step(t, -1).float().tolist()[2:4] == [0.0, 0.0] and bool(torch.isfinite(S.bf16_step(t, 1).float()).all())
    for case in (c for c in S.act_cases() if c.op == "swiglu"):
        emu = S.act_emulate(case)
        for scale in (1.0 + 2.0 ** -22, 1.0 - 2.0 ** -22):
            got = S.act_emulate(case, sigmoid_scale=scale)["a"]
            assert S.steps_from(got, emu["a"], case.name, floor=S.STEP_FLOOR, alternatives=emu["a_alt"]) == []
            plain = S.steps_from(got, emu["a"], case.name, floor=S.STEP_FLOOR)
            print(f"[row sweep] {case.name}: sigmoid x {scale:.8f}, against the plain emulation alone: {plain or 'within one step'}")


def test_an_rstd_off_in_its_last_bit_moves_a_cancelling_rope_sum_by_more_than_one_step():
    """Why the QK-norm + RoPE forward is compared from the kernel's own rstd: the same emulation with rstd one fp32 step up (another summation order does
    that) leaves the one-step band of the free-standing emulation on the large case, and is the emulation bit for bit once it is handed that rstd."""
    case = next(c for c in S.qk_cases() if c.form == "fwd" and c.tokens > 8192)
    emu = S.qk_emulate(case)
    up = torch.nextafter(emu["rstd"], torch.full_like(emu["rstd"], float("inf")))
    got = S.qk_emulate(case, rstd=up)
    d = (S.ordered(got["y"].reshape(-1)) - S.ordered(emu["y"].reshape(-1))).abs()
    print(f"[row sweep] {case.name}: rstd one fp32 step up: {int((d != 0).sum())} of {d.numel()} elements move, the farthest by {int(d.max())} bf16 steps")
    assert 0 < int((d != 0).sum()) <= S.STEP_SHARE * d.numel() and S.same_bits(S.qk_emulate(case, rstd=up)["y"], got["y"])
    judged, fails, _ = S.judge(got, S.qk_exact(case), case.name)
    assert not fails and judged == S.expected_units(case), "the fp64 bound holds either way"


def test_the_step_criterion_counts_steps_and_shares():
    a = torch.tensor([1.0, 2.0, -3.0, 0.0] * 250).to(BF16)
    assert S.steps_from(a, a.clone(), "x") == []
    b = a.clone()
    b[:2] = torch.tensor([1.0078125, 2.015625]).to(BF16)
    assert S.steps_from(b, a, "x") == [] and len(S.steps_from(torch.cat([b[:3], a[3:] * 1.0]), a, "x")) == 0
    b[:4] = torch.tensor([1.0078125, 2.015625, -3.015625, 0.0]).to(BF16)
    assert any("3 of 1000 elements differ" in f for f in S.steps_from(b, a, "x")), "three of a thousand exceed 2e-3"
    b = a.clone()
    b[5] = 2.03125
    assert any("2 bf16 steps" in f and "element 5" in f for f in S.steps_from(b, a, "x"))
