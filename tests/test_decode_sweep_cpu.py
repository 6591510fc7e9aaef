"""The judgement of the decode sweep (tests/decode_sweep.py) is sound: an fp32 emulation of attn_decode's order of operations passes it in every
case with every (sample, head) judged and reproduces every needle bit for bit, the measured c stays under its cap, the cases cover what they claim
to cover, and a defect planted in the emulation is named.  Runs without a GPU; prints the measured c per case."""

import pytest
import torch

import decode_sweep as S

BF16 = torch.bfloat16
GRID = S.grid_cases()
PEAKED = S.peaked_cases()
ALL = GRID + PEAKED + [S.WIDE_CASE]


@pytest.fixture(scope="module")
def tally():
    return {"c_raw": [], "c": [], "judged": 0, "cases": 0}


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_emulated_decode_attention_is_inside_the_bound(case, tally):
    ns, ex = S.build(case), S.exact(case)
    judged, fails, worst = S.judge(S.emulate(ns, case.splits), ex, case.name)
    S.report(case.name, ex, worst)
    assert ex.c_raw <= S.C_CAP, f"{case.name}: the fp32 reference alone needs c = {ex.c_raw:.3e} > 2^-10: wrong inputs for this test"
    assert S.C_FLOOR <= ex.c <= S.C_CAP
    assert not fails, "\n".join(fails)
    assert judged == ns.B * ns.Hq, "no (sample, head) is left out of the judgement"
    tally["c_raw"].append(ex.c_raw), tally["c"].append(ex.c)
    tally["judged"] += judged
    tally["cases"] += 1


def test_zz_range_of_c(tally):
    if tally["cases"] != len(ALL):
        pytest.skip("needs the whole module to have run")
    print(f"[decode sweep] attention: {tally['cases']} cases, {tally['judged']} (sample, head) pairs, 64 x fp32 reference error "
          f"{min(tally['c_raw']):.3e} .. {max(tally['c_raw']):.3e}, c {min(tally['c']):.3e} .. {max(tally['c']):.3e}")
    assert tally["judged"] == sum(S.BATCH * c.Hq for c in ALL) and max(tally["c"]) <= S.C_CAP


def test_operands_are_poisoned_and_laid_out_as_stated():
    for case in (GRID[0], GRID[13], GRID[39], PEAKED[0]):
        ns = S.build(case)
        q, kc, vc, km = S.views(ns)
        width = ns.Hkv * ns.D
        assert kc.stride() == vc.stride() == ((ns.cap + 3) * (width + 8), width + 8, 1) and kc.shape == (ns.B, ns.cap, width)
        for store, view in ((ns.ks, kc), (ns.vs, vc)):
            assert bool(torch.isfinite(view[:, : ns.L].float()).all()) and bool(torch.isnan(view[:, ns.L :].float()).all())
            assert int(torch.isfinite(store.float()).sum()) == ns.B * ns.L * width, "everything but the visible rows is NaN"
        if km is not None:
            assert km.stride(0) > ns.cap >= ns.host_len and int(ns.km_wide[:, ns.L :].sum()) == 0
            assert bool(((km[:, : ns.L] != 0) == ns.vis).all())
        assert ns.L == (ns.host_len if ns.len_dev is None else min(ns.host_len, ns.len_dev))
        assert {"host": ns.len_dev is None, "dev_equal": ns.len_dev == ns.host_len, "dev_shorter": ns.host_len == ns.cap and ns.len_dev == ns.L,
                "dev_longer": (ns.len_dev or 0) > ns.host_len}[case.source]
    holes = S.build(next(c for c in GRID if c.mask == "holes" and c.L > 60))
    assert set(holes.km_wide[:, : holes.L].unique().tolist()) == {0, 1, 2, 255}


# ----------------------------------------------------------------------------------------------------------------- needles
@pytest.mark.parametrize("D", list(S.GEOMETRY))
def test_needles_lead_by_30_nats_and_the_emulation_returns_their_value_rows(D):
    ns = S.build_needles(D)
    o64, _, s = S.softmax_reference(ns, torch.float64)
    lead = []
    for b, j in enumerate(ns.pos):
        others = torch.cat([s[b, :, :j], s[b, :, j + 1 :]], dim=-1)
        lead.append(float((s[b, :, j] - others.max(dim=-1).values).min()))
    print(f"[decode sweep] needles D{D}: {len(ns.pos)} positions, smallest lead {min(lead):.1f} nats")
    assert min(lead) >= 30.0
    assert S.same_bits(o64.to(BF16).view(ns.B, -1), ns.want), "the fp64 reference rounds to the needle's value row"
    for splits in (1, 3):
        assert S.same_bits(S.emulate(ns, splits), ns.want), f"splits {splits}"
    got = S.emulate(ns, 3, defect="swap_values")  # the needle at key 0 now meets value row 1
    wrong = [b for b in range(ns.B) if not S.same_bits(got[b], ns.want[b])]
    assert wrong == [ns.pos.index(0)] + ([ns.pos.index(1)] if 1 in ns.pos else [])


# ----------------------------------------------------------------------------------------------------------------- coverage
@pytest.mark.parametrize("D", list(S.GEOMETRY))
def test_the_cases_cover_what_they_claim(D):
    KG, NT, CK, ROUND = S.geometry(D)
    assert S.lengths(D) == (1, KG, KG + 1, CK - 1, CK, CK + 1, ROUND - 1, ROUND, ROUND + 1, 2 * ROUND + CK + KG + 1) and max(S.lengths(32)) == 1105
    pos = S.needle_positions(D)
    assert {0, KG - 1, KG, CK - 1, CK, 3 * CK - 1, 3 * CK, ROUND - 1, ROUND, ROUND + CK, S.longest(D) - 1} <= set(pos)
    marked = pos + [L - 1 for L in S.lengths(D)]  # the needles and the last key of every length
    one = [S.place(D, j, 1) for j in marked]
    assert {p["kg"] for p in one} == set(range(KG)) and {p["t"] for p in one} == set(range(NT))
    assert {p["wave"] for p in one} == set(range(S.WAVES)) and {p["trip"] for p in one} == {0, 1, 2}
    three = [S.place(D, j, 3) for j in marked]
    assert {p["split"] for p in three} == {0, 1, 2} and len({p["wave"] for p in three}) >= 6
    mine = [c for c in GRID if c.D == D]
    assert len(mine) == 10 and tuple(c.L for c in mine) == S.lengths(D) and len(GRID) == 40
    assert {(c.Hq, c.Hkv) for c in mine} == set(S.HEADS) and {c.splits for c in mine} == set(S.SPLITS)
    assert {c.source for c in mine} == set(S.SOURCES) and {c.mask for c in mine} == set(S.MASKS)
    assert any(c.splits > S.n_chunks(D, c.L) for c in mine), "a split that owns no key"
    assert any(1 < c.splits <= S.n_chunks(D, c.L) for c in mine), "several splits that all own keys"
    assert any(c.mask == "chunk" and c.L > c.splits * CK for c in mine), "a wave whose chunks are all masked beside visible ones"
    assert any(c.L > c.splits * ROUND for c in mine), "a wave that takes the prefetch path (a second trip of the key loop)"
    assert any(c.source == "dev_shorter" and c.L > CK for c in mine) and any(c.mask == "holes" and c.L > CK for c in mine)
    peaked = [c for c in PEAKED if c.D == D]
    assert sorted(c.splits for c in peaked) == [1, 3] and all(c.L == S.longest(D) and c.scale == 4.0 / D ** 0.5 for c in peaked)
    ns = S.build(peaked[0])
    _, _, s = S.softmax_reference(ns, torch.float64)
    assert bool((s[0, 0].diff() >= 0).all()) and bool((s[1, 0].diff() <= 0).all()), "head 0's scores ascend in sample 0 and descend in sample 1"


# ----------------------------------------------------------------------------------------------------------------- planted defects
def _case(**want):
    return next(c for c in GRID if all(getattr(c, k) == v for k, v in want.items()))


def _fails(case, defect, splits=None):
    ns, ex = S.build(case), S.exact(case)
    clean = S.judge(S.emulate(ns, splits or case.splits), ex, case.name)
    assert clean[:2] == (ns.B * ns.Hq, []), "the emulation without the defect passes"
    judged, fails, _ = S.judge(S.emulate(ns, splits or case.splits, defect=defect), ex, case.name)
    assert judged == ns.B * ns.Hq
    return fails


def test_the_judgement_names_a_dropped_last_key():
    for case in (_case(D=128, L=5), _case(D=64, L=65)):
        fails = _fails(case, "drop_last_key")
        assert fails and all("sample" in f and "head" in f for f in fails)


def test_the_judgement_names_two_swapped_value_rows():
    case = _case(D=64, L=63)
    assert len(_fails(case, "swap_values")) >= S.BATCH * case.Hq // 2


def test_the_judgement_names_a_wave_left_out_of_the_fold():
    case = _case(D=128, L=257)
    assert _fails(case, "skip_wave")


def test_the_judgement_names_an_empty_split_folded_with_weight_1():
    case = next(c for c in GRID if c.splits == 64 and c.L > 1 and c.splits > S.n_chunks(c.D, c.L))
    assert len(_fails(case, "empty_split_weight_1")) == S.BATCH * case.Hq


def test_the_judgement_names_one_head_of_sixteen_that_is_one_percent_off():
    case = S.WIDE_CASE
    ns, ex = S.build(case), S.exact(case)
    got = S.emulate(ns, 1, defect="scale_head")
    whole = S.rel_l2(got.float().view(ns.B, ns.Hq, ns.D), ex.ref)
    judged, fails, _ = S.judge(got, ex, case.name)
    print(f"[decode sweep] head 5 of sample 0 times 1.01: whole-tensor rel l2 {whole:.3e} (the old cap: 4e-3), per-head judgement: {fails[:1]}")
    assert whole < 4e-3, "the whole-tensor number of test_decode_gpu.py does not see it"
    assert judged == 32 and fails and all("sample 0, head 5" in f for f in fails)


def test_the_judgement_names_a_nan_from_a_row_past_the_length():
    for case in (_case(D=32, L=17), _case(D=256, L=128)):
        fails = _fails(case, "nan_past_len")
        assert fails and all("not finite" in f for f in fails)


# ----------------------------------------------------------------------------------------------------------------- gemv, argmax
@pytest.mark.parametrize("N,K", S.GEMV_SHAPES)
def test_gemv_bound_holds_for_an_fp32_accumulation_in_the_kernels_order(N, K):
    """512-element lane trips, 8 features per lane, then a butterfly over the 64 lanes -- in fp32, rounded once to bf16."""
    ns = S.gemv_case(N, K)
    for M in (1, 3, 8):
        for residual in (False, True):
            ex = S.gemv_exact(ns, M, residual)
            print(f"[decode sweep] gemv M{M} N{N} K{K} residual {int(residual)}: c = {ex.c:.3e} (64 x fp32 reference error {ex.c_raw:.3e})")
            assert ex.c_raw <= S.C_CAP
            prod = ns.x[:M].float()[:, None, :] * ns.w.float()[None, :, :]  # [M, N, K]
            pad = (-K) % 512
            lanes = torch.nn.functional.pad(prod, (0, pad)).view(M, N, -1, 64, 8)
            acc = torch.zeros(M, N, 64)
            for trip in range(lanes.shape[2]):
                for e in range(8):
                    acc = acc + lanes[:, :, trip, :, e]
            o = 32
            while o:
                acc = acc + acc.view(M, N, 64 // (2 * o), 2, o).flip(3).reshape(M, N, 64)
                o //= 2
            y = acc[:, :, 0] + (ns.r[:M].float() if residual else 0)
            label = f"gemv M{M} N{N} K{K}"
            assert not S.judge_gemv(y.to(BF16), ex, label)
            bad = y.clone()
            bad[M - 1, N - 1] *= 1.02  # one wrong column in up to 8 x 4099 outputs
            fails = S.judge_gemv(bad.to(BF16), ex, label)
            assert fails and f"row {M - 1}, column {N - 1}" in fails[0]


@pytest.mark.parametrize("V", S.ARGMAX_V)
def test_argmax_patterns_have_the_expected_answers(V):
    x, want, names, first = S.argmax_case(V)
    span = (V + 63) // 64
    assert len(want) == len(names) == x.shape[0] <= 300 and {"all -inf", "all NaN", "all equal", "all negative", "tie across a boundary"} <= set(names) | ({"tie across a boundary"} if V == 1 else set())
    for r, w, n in zip(x, want, names):
        if n in ("all -inf", "all equal"):
            assert w == 0
        if w == S.IN_RANGE:
            assert bool(torch.isnan(r).any())
        else:
            assert w == int(torch.argmax(r.float())) or n == "tie across a boundary" or n == "all equal" or n == "all -inf"
            assert float(r[w]) == float(r.float().max()) and (w == 0 or float(r[:w].float().max()) < float(r[w]))
    planted = {w for w, n in zip(want, names) if n == "max at a range edge"}
    assert {0, V - 1} <= planted and all(i in planted for k in range(1, 64) for i in (k * span - 1, k * span) if i < V)
