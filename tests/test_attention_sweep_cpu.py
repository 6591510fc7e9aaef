"""The bound of the attention sweep (tests/attention_sweep.py) is one a correct flash-form kernel meets: an fp32 emulation of the kernels' rounding
points (bf16 operands, P and dS rounded to bf16, bf16 outputs, the scale folded into a bf16 operand or not) stays inside it in every block of a
subset of the GPU grid, and no block is excluded from the judgement.  Runs without a GPU."""

import pytest
import torch

import attention_sweep as A

# every length of the grid that sits on or next to a 32-, 64- or 128-token edge below 200, and one two-block length; the head shapes and the mask
# kinds rotate as in the GPU grid
CPU_CASES = [c for c in A.sweep_cases() if c[1] in (1, 31, 33, 64, 65, 127, 129, 193, 257)]


@pytest.fixture(scope="module")
def tally():
    return {"judged": 0, "total": 0, "cases": 0, "worst": {False: 0.0, True: 0.0}}


@pytest.mark.parametrize("case", CPU_CASES, ids=A.case_id)
def test_emulated_flash_attention_is_inside_the_sweeps_bound(case, tally):
    B, S, Hq, Hkv, D, causal, mask = case
    q, k, v, do = A.operands(B, S, Hq, Hkv, D, seed=S * 131 + Hq * 17 + D + causal)
    km = A.key_mask(mask, B, S)
    dead = A.fully_masked_rows(B, S, km, causal)
    if bool(dead.any()):  # the backward's contract: it equals the reference where dO is zero on fully-masked rows
        do = do.masked_fill(dead[:, None, :, None], 0.0)
    exact = A.reference(q, k, v, do, km, causal, torch.float64)
    floor = A.reference(q, k, v, do, km, causal)
    for fold in (False, True):
        got = A.emulate(q, k, v, do, km, causal, fold)
        worst, judged, total, fails = A.judge(got, exact, floor, km, causal, (q, k, v, do))
        w, w1, f = A.judge_lse(got["lse"], q, k, km, causal)
        A.report(f"{A.case_id(case)} fold={int(fold)} |dlse| {w:.1e} (one-key rows {w1:.1e})", worst)
        assert not fails + f, "\n".join(fails + f)
        assert judged == total == A.n_blocks(B, Hq, S) * 2 + A.n_blocks(B, Hkv, S) * 2, "no block is left out of the judgement"
        tally["judged"] += judged
        tally["total"] += total
        tally["worst"][fold] = max(tally["worst"][fold], max(worst.values()))
    tally["cases"] += 1


def test_zz_no_block_of_the_subset_was_excluded(tally):
    """Runs after the cases above: what they judged is everything there is."""
    if tally["cases"] != len(CPU_CASES):
        pytest.skip("needs the whole module to have run")
    want = sum(2 * (A.n_blocks(B, Hq, S) * 2 + A.n_blocks(B, Hkv, S) * 2) for B, S, Hq, Hkv, D, causal, mask in CPU_CASES)
    print(f"[attention sweep] {tally['cases']} cases, {tally['judged']} blocks, worst ratio {tally['worst'][False]:.3f} without the fold, {tally['worst'][True]:.3f} with it")
    assert tally["judged"] == tally["total"] == want


def test_block_edges_cover_every_token_once():
    for S in range(1, 200):
        e = A.block_edges(S)
        assert e[0][0] == 0 and e[-1][1] == S and all(a[1] == b[0] for a, b in zip(e, e[1:]))
        assert all(b - a == 32 for a, b in e[:-1]) and (S < 32 or 32 <= e[-1][1] - e[-1][0] < 64)


def test_the_judgement_catches_one_wrong_block_and_one_missing_store():
    """A 32-row slice that is 3 % off, hidden under the whole-tensor number, and a row left at zero or NaN are both named."""
    B, S, Hq, Hkv, D = 1, 257, 2, 1, 64
    q, k, v, do = ops = A.operands(B, S, Hq, Hkv, D, seed=5)
    exact = A.reference(q, k, v, do, None, True, torch.float64)
    floor = A.reference(q, k, v, do, None, True)
    got = A.emulate(q, k, v, do, None, True, False)
    bad = {n: t.clone() for n, t in got.items()}
    bad["dq"][0, 1, 96:128] = (bad["dq"][0, 1, 96:128].float() * 1.03).to(A.BF16)
    assert A.rel_l2(bad["dq"], exact["dq"]) < A.CAP["dq"], "the whole-tensor number does not see it"
    fails = A.judge(bad, exact, floor, None, True, ops)[3]
    assert len(fails) == 1 and "dq: sample 0, head 1, block 3" in fails[0], fails
    bad = {n: t.clone() for n, t in got.items()}
    bad["dv"][0, 0, 200] = float("nan")
    assert "not finite" in A.judge(bad, exact, floor, None, True, ops)[3][0]
    km = A.key_mask("right", B, S)
    exact = A.reference(q, k, v, do, km, True, torch.float64)
    got = A.emulate(q, k, v, do, km, True, True)
    assert not A.judge(got, exact, A.reference(q, k, v, do, km, True), km, True, ops)[3]
    got["dk"][0, 0, S - 1, 3] = 1e-30  # a padded key
    assert "must be exactly 0" in A.judge(got, exact, A.reference(q, k, v, do, km, True), km, True, ops)[3][0]
