"""The sweep of the side attention families (tests/side_attention_sweep.py) without a GPU: the honest fp32 emulation of the kernels' rounding points
passes the judgement on every case of the three tables with every block judged; the tables reach every branch of the kernels per head-dim pair; the
generalised one-key rule returns what it returned before; and fifteen planted faults, each one expression changed in the emulation, are caught and
named -- with the whole-tensor number the older tests would have seen printed next to each."""

import pytest
import torch

import attention_sweep as A
import deepseek_oracle as DO
import side_attention_sweep as X

ALL_CASES = X.band_cases() + X.ga_cases() + X.mla_cases()


@pytest.fixture(scope="module")
def tally():
    return {"judged": 0, "total": 0, "cases": 0}


# ----------------------------------------------------------------------------------------------------------------- the honest emulation
@pytest.mark.parametrize("case", ALL_CASES, ids=[X.family_of(c) + "-" + X.case_id(c) for c in ALL_CASES])
def test_honest_emulation_is_inside_the_bound_in_every_block(case, tally):
    ops = {"band": X.band_operands, "ga": X.ga_operands, "mla": X.mla_operands}[X.family_of(case)](case)
    exact, floor = X.reference(case, ops)
    worst, judged, total, fails = X.judge_case(case, X.emulate(case, ops), exact, floor, ops)
    X.report(f"{X.family_of(case)} {X.case_id(case)}", worst)
    assert not fails, "\n".join(fails)
    assert judged == total == X.blocks_of(case), "no block is left out of the judgement"
    X.note(tally, case, worst)
    tally["judged"] += judged
    tally["total"] += total
    tally["cases"] += 1


def test_zz_worst_ratio_of_the_emulation_and_the_block_count(tally):
    """Runs after the cases above: what they judged is everything there is; prints the CPU column of side_attention_sweep.MEASURED."""
    if tally["cases"] != len(ALL_CASES):
        pytest.skip("needs the whole module to have run")
    for fam in ("band", "ga", "mla"):
        X.report(f"emulation, {fam}, all cases", tally[fam])
        assert max(tally[fam].values()) <= 1.0
    want = sum(X.blocks_of(c) for c in ALL_CASES)
    print(f"[side attention sweep] {tally['cases']} cases, {tally['judged']} blocks")
    assert tally["judged"] == tally["total"] == want


# ----------------------------------------------------------------------------------------------------------------- the tables
def test_the_tables_are_the_stated_grids():
    band = X.band_cases()
    assert {c.S for c in band} == set(X.BAND_S) and max(c.S for c in ALL_CASES) <= 385
    assert all(c.B == (2 if c.S <= 200 else 1) for c in ALL_CASES)
    for S in X.BAND_S:
        ws = {c.W for c in band if c.S == S}
        assert {w for w in X.BAND_W + (S - 1, S) if 1 <= w <= S} <= ws and len([w for w in ws if w > S]) == 1, S
    assert {c.W for c in band} >= {X.W_HUGE}
    for pair in X.BAND_PAIRS:
        cs = [c for c in band if (c.D, c.DV) == pair]
        assert {(c.Hq, c.Hkv) for c in cs} == set(X.BAND_HEADS)
        if pair == (32, 32):
            assert all(c.entry == "swa" and c.sink is None for c in cs)
            continue
        assert [c.sink for c in cs].count("low") == 1 and [c.sink for c in cs].count("high") == 1 and any(c.sink == "rand" for c in cs)
        assert any(c.sink is None for c in cs)
        if pair[0] == pair[1]:  # DV = D without a sink: both entry points
            assert {c.entry for c in cs if c.sink is None} == {"swa", "sink"}
    assert all(c.entry == "sink" for c in band if c.sink is not None or c.D != c.DV)
    ga = X.ga_cases()
    assert {(c.S, c.D) for c in ga} == {(S, D) for S in A.SWEEP_S for D in X.GA_D} and len(ga) == 64
    for D in X.GA_D:
        assert {c.mode for c in ga if c.D == D} == set(X.GA_MODES) and {(c.Hq, c.Hkv) for c in ga if c.D == D} == set(X.GA_HEADS)
    mla = X.mla_cases()
    assert {(c.S, c.Dn, c.Dr) for c in mla} == {(S, *d) for S in A.SWEEP_S for d in X.MLA_DIMS}
    for d in X.MLA_DIMS:
        cs = [c for c in mla if (c.Dn, c.Dr) == d]
        assert {c.Hq for c in cs} == set(X.MLA_HEADS) and {c.sliced for c in cs} == {True, False}
    assert len(set(ALL_CASES)) == len(ALL_CASES)


def test_every_branch_is_taken_by_a_case_of_every_pair():
    for pair in X.BAND_PAIRS:
        took = [X.band_branches(c) for c in X.band_cases() if (c.D, c.DV) == pair]
        for b in X.BAND_BRANCHES:
            assert any(t[b] for t in took), (pair, b)
    for D in X.GA_D:
        took = [X.ga_branches(c) for c in X.ga_cases() if c.D == D]
        for b in X.GA_BRANCHES:
            assert any(t[b] for t in took) == (b != "NP = 2" or D == 256), (D, b)
    for d in X.MLA_DIMS:
        took = [X.mla_branches(c) for c in X.mla_cases() if (c.Dn, c.Dr) == d]
        for b in X.MLA_BRANCHES:
            assert any(t[b] for t in took) == (b != "NP = 2" or d == (128, 64)), (d, b)


def test_the_branch_predicates_on_cases_worked_by_hand():
    bc = lambda S, W, Hq=2, Hkv=2: X.band_branches(X.BandCase(1, S, Hq, Hkv, 64, 64, W, None, "swa"))
    t = bc(257, 2)  # workgroup 2 is query 256 alone; kfirst = 255 lies in the 128-block before it; wave 1 of workgroup 0 walks tile 0 for row 32 only
    assert t[X.BAND_BRANCHES[0]] and t[X.BAND_BRANCHES[1]] and t[X.BAND_BRANCHES[2]] and t[X.BAND_BRANCHES[3]] and t[X.BAND_BRANCHES[4]] and t[X.BAND_BRANCHES[5]]
    assert t[X.BAND_BRANCHES[7]] and t[X.BAND_BRANCHES[8]] and t[X.BAND_BRANCHES[9]] and not t[X.BAND_BRANCHES[10]]
    t = bc(128, 1)  # aligned, a window of one: every wave walks its diagonal tile only
    assert not t[X.BAND_BRANCHES[0]] and not t[X.BAND_BRANCHES[3]] and not t[X.BAND_BRANCHES[4]] and not t[X.BAND_BRANCHES[5]] and t[X.BAND_BRANCHES[1]]
    t = bc(64, 2 ** 40, 6, 2)  # plain causal on two waves
    assert not t[X.BAND_BRANCHES[1]] and t[X.BAND_BRANCHES[2]] and t[X.BAND_BRANCHES[6]] and not t[X.BAND_BRANCHES[7]] and not t[X.BAND_BRANCHES[9]] and t[X.BAND_BRANCHES[10]]
    g = X.ga_branches(X.GaCase(2, 31, 2, 1, 256, "quirk-right"))
    assert g == {"all_keys on": True, "all_keys off": False, "NP = 2": True, "a padded key inside the causal triangle": True, "a padded key outside the causal triangle": True}
    assert X.ga_branches(X.GaCase(2, 31, 2, 1, 64, "plain-causal"))["all_keys off"]


# ----------------------------------------------------------------------------------------------------------------- the generalised one-key rule
def _one_key_bounds_before(q, k, v, do, km, causal):
    """attention_sweep.one_key_bounds as it stood before it took an allowed-pairs matrix."""
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    src = torch.arange(Hq) // (Hq // Hkv)
    seen = ~A.blocked_pairs(B, S, km, causal)[:, 0]
    rows = seen.sum(dim=-1) == 1
    j = seen.int().argmax(dim=-1)[:, None, :, None].expand(B, Hq, S, D)
    kj, vj = k.double()[:, src].gather(2, j), v.double()[:, src].gather(2, j)
    ds = 2.0 ** -7 * D ** -0.5 * (do.double() * vj).abs().sum(dim=-1, keepdim=True)
    out = {"dq": (rows[:, None, :].expand(B, Hq, S), ds * kj.abs())}
    if S == 1:
        out["dk"] = (rows[:, None, :].expand(B, Hkv, S), (ds * q.double().abs()).view(B, Hkv, Hq // Hkv, S, D).sum(dim=2))
    return out


def test_one_key_bounds_returns_what_it_did_for_every_case_of_the_tuned_sweep():
    for B, S, Hq, Hkv, D, causal, mask in A.sweep_cases():
        ops = A.operands(B, S, Hq, Hkv, D, seed=S + Hq + D)
        km = A.key_mask(mask, B, S)
        old, new = _one_key_bounds_before(*ops, km, causal), A.one_key_bounds(*ops, km, causal)
        assert old.keys() == new.keys(), (S, mask, causal)
        for name in old:
            assert torch.equal(old[name][0], new[name][0]) and torch.equal(old[name][1], new[name][1]), (name, S, mask, causal)
        again = A.one_key_bounds(*ops, None, False, ~A.blocked_pairs(B, S, km, causal)[:, 0])  # the same mask as an explicit matrix
        assert all(torch.equal(old[n][0], again[n][0]) and torch.equal(old[n][1], again[n][1]) for n in old)


def test_a_window_of_one_has_one_key_rows_and_one_query_keys_everywhere():
    c = X.BandCase(2, 65, 6, 2, 64, 32, 1, None, "sink")
    ops = X.band_operands(c)
    exact, floor = X.reference(c, ops)
    assert float(exact["dq"].abs().max()) == 0.0 and float(exact["dk"].abs().max()) == 0.0
    b = A.one_key_bounds(*ops[:4], None, False, X.allowed_of(c))
    assert bool(b["dq"][0].all()) and bool(b["dk"][0].all())
    got = X.emulate(c, ops)
    assert not X.judge_case(c, got, exact, floor, ops)[3]
    got["dk"][1, 0, 40, 3] = 1.0  # far above one rounding of o
    assert "one-key row" in X.judge_case(c, got, exact, floor, ops)[3][0]
    # the tuned sweep's judge takes the same matrix
    w, judged, total, fails = A.judge({n: got[n] for n in ("dq", "dv")}, exact, floor, None, False, ops[:4], allowed=X.allowed_of(c))
    assert not fails and judged == total
    # with a sink nothing is a one-key row, and nothing is zero
    c = c._replace(sink="rand")
    ops = X.band_operands(c)
    exact, floor = X.reference(c, ops)
    assert X._one_key(c, ops) == {} and not X.judge_case(c, X.emulate(c, ops), exact, floor, ops)[3]


def test_per_head_shares_of_the_shared_rotary_key_sum_to_its_gradient():
    for c in (X.MlaCase(2, 33, 3, 64, 32, False), X.MlaCase(1, 65, 2, 128, 64, False)):
        ops = X.mla_operands(c)
        exact, floor = X.reference(c, ops)
        whole = DO.mla_attention_bwd(*ops[:5], ops[5], dtype=torch.float64)
        assert torch.allclose(exact["dk_rope_heads"].sum(dim=1), whole[3], rtol=1e-12, atol=1e-14)
        for name, g in zip(("dq_nope", "dq_rope", "dk_nope", None, "dv"), whole):
            assert name is None or torch.allclose(exact[name], g, rtol=1e-12, atol=1e-14), name
        assert A.rel_l2(floor["dk_rope_heads"].sum(dim=1), whole[3]) < 0.1


# ----------------------------------------------------------------------------------------------------------------- planted faults
# Which cases a fault runs on is fixed here, from the case (and its operands) alone, before any result:
#   window faults (too wide, too narrow, first tile): every (D, DV) pair, S >= W + 32 and W <= 129, so that at least 32 rows have a full window with a key
#       in front of it; the first-tile fault also needs W >= 2 (at W = 1 a band is one key and lies in the row's own tile);
#   sink faults: W <= 129 and a sink that carries weight in the first block, where a row has 1 .. 32 keys: +30, or N(0, 1) logits with a head at z >= 1
#       (e^z against about 1.65 x keys: more than 5 % of the mass of the first block's rows); the sink of -30000 is exactly inert.  The live-sink
#       cases the rule leaves out (every head's z below 1) run too and are reported, not asserted: the table records where a weak sink hides these faults;
#   dsink's dropped partial row: a live sink at W <= 129 and B S <= 256, where the one workgroup's row is the whole sum and dsink comes back 0; it is
#       named by its head.  With more workgroups the last one may hold as few as 2 of 258 rows (S = 129), less than the roundings of the other 256:
#       those cases run too and are reported, not asserted;
#   head mapping: 1 < Hkv < Hq, the only shapes where h % Hkv and h / rep differ;
#   quirk: a key mask with a padded key;  PLAIN full as causal: S >= 2;  slices: every case at D = 256 and at (128, 64);
#   rope half: every mla case;  k_rope not shared: Hq >= 2 and S >= 2;  ragged row: S % 32 != 0 (and the band rule's W <= 129).
def _window_rule(c):
    return c.S >= c.W + 32 and c.W <= 129


def _live_sink(c, ops):
    return c.W <= 129 and c.sink in ("rand", "high")


def _sink_rule(c, ops):
    return _live_sink(c, ops) and (c.sink == "high" or float(ops[4].max()) >= 1.0)


SINK_FAULTS = ("sink left out of l", "sink multiplied by the scale", "sink absent from the backward's lse", "last partial row of dsink dropped")


RULES = {
    "window one too wide": lambda c, ops: _window_rule(c),
    "window one too narrow": lambda c, ops: _window_rule(c),
    "first tile of a row's band dropped": lambda c, ops: _window_rule(c) and c.W >= 2,
    "sink left out of l": _sink_rule,
    "sink multiplied by the scale": _sink_rule,
    "sink absent from the backward's lse": _sink_rule,
    "query head mapped to h % Hkv": lambda c, ops: c.W <= 129 and 1 < c.Hkv < c.Hq,
    "last partial row of dsink dropped": lambda c, ops: _live_sink(c, ops) and c.B * c.S <= 256,
    "quirk dropped, padded keys masked": lambda c, ops: X.ga_key_mask(c) is not None and not bool(X.ga_key_mask(c).all()),
    "PLAIN full run as causal": lambda c, ops: c.mode == "plain-full" and c.S >= 2,
    "second dK/dV slice at D = 256 unstored": lambda c, ops: c.D == 256,
    "rope half of the score dropped": lambda c, ops: True,
    "k_rope not shared": lambda c, ops: c.Hq >= 2 and c.S >= 2,
    "second dK/dV slice at (128, 64) unstored": lambda c, ops: (c.Dn, c.Dr) == (128, 64),
    "ragged tile row read as its neighbour": lambda c, ops: c.S % 32 != 0 and (not isinstance(c, X.BandCase) or c.W <= 129),
}


def _old_whole_tensor_verdict(c, got, exact, floor):
    """The worst whole-tensor rel_l2 of the faulty result over its bound in the older tests: 1.5 x floor + 2e-3 (band, mla: test_gemma3_gpu.judge), fixed
    6e-3 forward / 1e-2 backward (ga: test_qwen35_text_gpu.py).  -> (tensor, rel_l2, bound) of the worst, NaN counted as seen."""
    worst = None
    for name in X.NAMES[X.family_of(c)] + (("dsink",) if "dsink" in got else ()):  # dsink as the [Hq] vector, the way test_mimo_gpu.py judged it
        if not bool(torch.isfinite(got[name].float()).all()):
            return name, float("nan"), 0.0
        if float(exact[name].norm()) == 0.0:
            continue
        e, fl = A.rel_l2(got[name], exact[name]), A.rel_l2(floor[name], exact[name])
        bound = (6e-3 if name == "o" else 1e-2) if isinstance(c, X.GaCase) else 1.5 * fl + (0.0 if fl >= 1e-2 else 2e-3)
        if worst is None or e / bound > worst[1] / worst[2]:
            worst = (name, e, bound)
    return worst


@pytest.mark.parametrize("family", ["band", "ga", "mla"])
def test_planted_faults_are_caught_and_named(family):
    cases = {"band": X.band_cases, "ga": X.ga_cases, "mla": X.mla_cases}[family]()
    build = {"band": X.band_operands, "ga": X.ga_operands, "mla": X.mla_operands}[family]
    faults = [f for f, fam in X.FAULTS.items() if fam in (family, "all")]
    table = {f: {"ran": 0, "caught": 0, "old passes": 0, "pairs": set(), "example": None, "missed": [], "least": None} for f in faults}
    weak = {f: [0, 0] for f in SINK_FAULTS}  # live-sink cases outside the rule: run, caught
    for c in cases:
        ops = build(c)
        todo = [f for f in faults if RULES[f](c, ops)]
        extra = [f for f in SINK_FAULTS if family == "band" and f not in todo and _live_sink(c, ops)]
        if not todo + extra:
            continue
        exact, floor = X.reference(c, ops)
        for f in extra:
            weak[f][0] += 1
            weak[f][1] += bool(X.judge_case(c, X.emulate(c, ops, f), exact, floor, ops)[3])
        for f in todo:
            got = X.emulate(c, ops, f)
            fails = X.judge_case(c, got, exact, floor, ops)[3]
            named = [x for x in fails if "block" in x or "token" in x or (f.startswith("last partial row of dsink") and "dsink: head" in x)]
            row = table[f]
            row["ran"] += 1
            row["pairs"].add((c.D, c.DV) if family == "band" else c.D if family == "ga" else (c.Dn, c.Dr))
            if named:
                row["caught"] += 1
            else:
                row["missed"].append(X.case_id(c))
            name, e, bound = _old_whole_tensor_verdict(c, got, exact, floor)
            if e == e and (row["least"] is None or e / bound < row["least"][0]):  # the case where the old bound sees the fault least (NaN aside)
                row["least"] = (e / bound, f"{name} rel_l2 {e:.2e} against the old bound {bound:.2e} ({X.case_id(c)})")
            if e <= bound:
                row["old passes"] += 1
                row["example"] = row["example"] or f"{X.case_id(c)}: {name} whole-tensor rel_l2 {e:.2e} <= old bound {bound:.2e}; the sweep says: {named[0] if named else '-'}"
    print(f"\n[side attention sweep] planted faults, {family}: cases run / caught block by block / passed by the old whole-tensor bound")
    for f, row in table.items():
        print(f"  {f:45s} {row['ran']:3d} / {row['caught']:3d} / {row['old passes']:3d}   whole tensor, least visible: "
              + (row["least"][1] if row["least"] else "NaN in every case") + (f"   passed e.g. {row['example']}" if row["example"] else ""))
    if family == "band":
        for f, (ran, caught) in weak.items():
            print(f"  {f:45s} live sinks outside the rule: {ran} run, {caught} caught, {ran - caught} hidden (not asserted)")
    for f, row in table.items():
        assert row["ran"] > 0, f"{f}: the rule selects no case"
        assert not row["missed"], f"{f}: not caught on {row['missed']}"
    for f in ("window one too wide", "window one too narrow", "first tile of a row's band dropped"):
        if f in table:
            assert table[f]["pairs"] == set(X.BAND_PAIRS), f"{f}: every pair"


# ----------------------------------------------------------------------------------------------------------------- the two derived bounds
def test_the_derived_bounds_are_what_the_emulation_shows():
    """side_attention_sweep.py, "Derived bounds": the honest emulation misses the plain rule exactly in the two classes that have a derived bound,
    lands where the derivation says, and stays inside the derived bound.  Prints the figures quoted in the module docstring."""
    heads = missed = 0
    sigmas, blocks_over, worst_plain, worst_derived, block_sigmas, kept_plain, blocks = [], 0, 0.0, 0.0, [], 0, 0
    for c in X.band_cases():
        if c.sink not in ("rand", "high"):
            continue
        ops = X.band_operands(c)
        exact, floor = X.reference(c, ops)
        got = X.emulate(c, ops)
        err = (got["dsink"].double() - exact["dsink"].double()).abs()
        fl = (floor["dsink"].double() - exact["dsink"].double()).abs() / exact["dsink"].double().abs()
        plain = 1.5 * fl + torch.where(fl >= 1e-2, 0.0, 2e-3)
        heads += c.Hq
        missed += int((err / exact["dsink"].double().abs() > plain).sum())
        sigmas += (err / X.dsink_sigma(c, ops, exact)).tolist()
        caps = X.one_key_sink_caps(c, ops, exact)
        for name, cap in caps.items():
            e = (A._block_norms(got[name].double() - exact[name].double(), c.S) / A._block_norms(exact[name].double(), c.S)).sqrt()
            block_sigmas += (e / X.one_key_sink_sigma(c, ops, exact)[name]).flatten().tolist()
            kept_plain += int((cap == X.GRAD_CAP).sum())
            blocks += cap.numel()
            f = (A._block_norms(floor[name].double() - exact[name].double(), c.S) / A._block_norms(exact[name].double(), c.S)).sqrt()
            over = e > torch.maximum(1.5 * f, torch.full_like(f, X.GRAD_CAP))
            blocks_over += int(over.sum())
            if bool(over.any()):
                worst_plain = max(worst_plain, float(e[over].max()))
                worst_derived = max(worst_derived, float((e / cap)[over].max()))
    s = torch.tensor(sigmas)
    print(f"\n[side attention sweep] dsink: {heads} heads, {missed} miss the 1.5x rule alone; |error| / sigma: worst {float(s.max()):.2f}, median {float(s.median()):.2f}")
    b = torch.tensor(block_sigmas)
    print(f"[side attention sweep] one key and a sink: {blocks} blocks of dq / dk, {kept_plain} keep the plain cap, {blocks_over} of the emulation are over the "
          f"plain bound, worst rel l2 {worst_plain:.2e} = {worst_derived:.2f} of the derived bound; error norm / sigma: worst {float(b.max()):.2f}, median {float(b.median()):.2f}")
    assert missed > 0 and blocks_over > 0, "the plain rule would do: drop the derived bound"
    assert 1.0 <= float(s.max()) <= X.DSINK_SIGMAS, "the model is neither vacuous nor exceeded"
    # the block model is a fit, not an upper bound: the emulation lands ON its sigma in the median and stays inside the stated multiple
    assert 0.8 <= float(b.median()) <= 1.2 and 1.0 <= float(b.max()) <= X.ONE_KEY_SINK_SIGMAS
    assert 0.5 <= worst_derived <= 1.0
