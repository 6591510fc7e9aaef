"""The attention forward and backward of csrc/attention.hip against fp64 on a real MI355X, block by block (tests/attention_sweep.py): lengths on
and next to every 32-, 64- and 128-token edge, GQA ratios 1 to 8, both head dims, both backward forms, the four mask kinds, strided operands, the
persistent walks at small S, and left padding in the backward.  Gradient buffers are pre-filled with NaN: a row the kernel never stores is seen.
Every case prints its worst block ratio (kernel / bound) per tensor; the last test prints the worst per form."""

import pytest
import torch

import attention_sweep as A

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FORMS = {128: ("spill", "recompute"), 64: ("recompute",)}  # the dS-spill form is built for head_dim 128


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import kernels

    return kernels


@pytest.fixture(scope="module")
def tally():
    return {}


def _note(tally, form, D, worst):
    row = tally.setdefault("D = 64" if D == 64 else form, {})
    for n, w in worst.items():
        row[n] = max(row.get(n, 0.0), w)


def _nan(t):
    return torch.full_like(t, float("nan"))


def _backward(K, form, q, k, v, o, do, lse, B, S, Hq, Hkv, D, dq, dk, dv, km, causal):
    """``attn_bwd`` in the given form; asserts through ``attn_bwd_form`` that this form ran."""
    keep, before = K._ATTN_DS_SPILL, dict(K.attn_bwd_form)
    K._ATTN_DS_SPILL = form == "spill"
    try:
        K.attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, dq, dk, dv, key_mask=km, causal=causal)
    finally:
        K._ATTN_DS_SPILL = keep
    other = "recompute" if form == "spill" else "spill"
    assert K.attn_bwd_form[form] == before[form] + 1 and K.attn_bwd_form[other] == before[other], f"the {form} form did not run"


def _forward(K, ops4, km, causal):
    """[B, H, S, D] CPU operands -> device token-major operands, o, lse."""
    q4, k4, v4, do4 = ops4
    B, Hq, S, D = q4.shape
    q, k, v, do = (A.to_tokens(t).cuda() for t in ops4)
    kmd = None if km is None else km.cuda()
    o, lse = K.attn_fwd(q, k, v, B, S, Hq, k4.shape[1], D, key_mask=kmd, causal=causal)
    return q, k, v, do, kmd, o, lse


def _grads(K, form, dev, shape, causal):
    q, k, v, do, kmd, o, lse = dev
    B, S, Hq, Hkv, D = shape
    dq, dk, dv = _nan(q), _nan(k), _nan(v)
    _backward(K, form, q, k, v, o, do, lse, B, S, Hq, Hkv, D, dq, dk, dv, kmd, causal)
    return {"dq": A.from_tokens(dq.cpu(), B, S, Hq, D), "dk": A.from_tokens(dk.cpu(), B, S, Hkv, D), "dv": A.from_tokens(dv.cpu(), B, S, Hkv, D)}


def _check(label, got, exact, floor, km, causal, ops4, blocks):
    worst, judged, total, fails = A.judge(got, exact, floor, km, causal, ops4)
    A.report(label, worst)
    assert not fails, label + "\n" + "\n".join(fails)
    assert judged == total == blocks, "no block is left out of the judgement"
    return worst


# ----------------------------------------------------------------------------------------------------------------- the edge grid
@pytest.mark.parametrize("case", A.sweep_cases(), ids=A.case_id)
def test_attention_edge_grid_matches_fp64_block_by_block(K, case, tally):
    """Forward (o, lse) and backward (both forms at D = 128) of one case of the grid.  Where the mask leaves fully-masked rows (``left`` under the
    causal mask) dO is zero on them: the backward's contract (test_attention_backward_left_padding pins what happens otherwise)."""
    B, S, Hq, Hkv, D, causal, mask = case
    ops4 = list(A.operands(B, S, Hq, Hkv, D, seed=S * 131 + Hq * 17 + D + causal))
    km = A.key_mask(mask, B, S)
    dead = A.fully_masked_rows(B, S, km, causal)
    if bool(dead.any()):
        ops4[3] = ops4[3].masked_fill(dead[:, None, :, None], 0.0)
    exact = A.reference(*ops4, km, causal, torch.float64)
    floor = A.reference(*ops4, km, causal)
    dev = _forward(K, ops4, km, causal)
    o, lse = dev[5], dev[6]
    nq, nk = A.n_blocks(B, Hq, S), A.n_blocks(B, Hkv, S)
    w = _check(f"{A.case_id(case)} forward", {"o": A.from_tokens(o.cpu(), B, S, Hq, D)}, exact, floor, km, causal, ops4, nq)
    d, d1, fails = A.judge_lse(lse.cpu(), ops4[0], ops4[1], km, causal)
    print(f"[attention sweep] {A.case_id(case)} max |lse - ref| {d:.2e} (one-key rows {d1:.2e})")
    assert not fails, fails
    tally.setdefault("lse", {"several keys": 0.0, "one key": 0.0})
    tally["lse"] = {"several keys": max(tally["lse"]["several keys"], d), "one key": max(tally["lse"]["one key"], d1)}
    for form in FORMS[D]:
        _note(tally, form, D, w)
        g = _grads(K, form, dev, (B, S, Hq, Hkv, D), causal)
        _note(tally, form, D, _check(f"{A.case_id(case)} {form}", g, exact, floor, km, causal, ops4, nq + 2 * nk))


def test_zz_worst_block_ratio_per_form(tally):
    """Runs after the grid: the table of DESIGN.md section 4 (worst block ratio per tensor and form over the edge grid)."""
    if not tally:
        pytest.skip("needs the grid to have run")
    lse = tally.pop("lse")
    print(f"[attention sweep] edge grid, max |lse - ref|: {lse['several keys']:.2e} on rows with several keys, {lse['one key']:.2e} on one-key rows")
    for form, row in tally.items():
        A.report(f"edge grid, {form}", row)
        assert max(row.values()) <= 1.0
    tally["lse"] = lse


# ----------------------------------------------------------------------------------------------------------------- strided operands
@pytest.mark.parametrize("D", [64, 128])
def test_attention_backward_on_column_slices_of_fused_buffers(K, D):
    """q, k, v are column slices of one fused buffer and dq, dk, dv of another (row pitch = the fused width plus a margin on either side): the same
    bits as the packed run, and the columns of the destination that belong to no gradient are unchanged."""
    B, S, Hq, Hkv, causal = 2, 193, 4, 2, True
    ops4 = A.operands(B, S, Hq, Hkv, D, seed=D + 3)
    km = A.key_mask("holes", B, S)
    q, k, v, do, kmd, o, lse = _forward(K, ops4, km, causal)
    packed = _nan(q), _nan(k), _nan(v)
    K.attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, *packed, key_mask=kmd, causal=causal)
    nq, nk, pad = Hq * D, Hkv * D, 8
    cols = [pad, pad + nq, pad + nq + nk, pad + nq + 2 * nk]
    g = torch.Generator().manual_seed(9)
    src = torch.randn(B * S, cols[3] + pad, generator=g).to(BF16).cuda()
    for t, a, b in zip((q, k, v), cols, cols[1:]):
        src[:, a:b] = t
    fill = torch.randn(B * S, cols[3] + pad, generator=g).to(BF16).cuda()
    dst = fill.clone()
    for a, b in zip(cols, cols[1:]):
        dst[:, a:b] = float("nan")
    views = [src[:, a:b] for a, b in zip(cols, cols[1:])]
    o2, lse2 = K.attn_fwd(*views, B, S, Hq, Hkv, D, key_mask=kmd, causal=causal)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    K.attn_bwd(*views, o, do, lse, B, S, Hq, Hkv, D, *[dst[:, a:b] for a, b in zip(cols, cols[1:])], key_mask=kmd, causal=causal)
    for name, want, a, b in zip(("dq", "dk", "dv"), packed, cols, cols[1:]):
        assert torch.isfinite(want.float()).all() and torch.equal(dst[:, a:b], want), name
    assert torch.equal(dst[:, :pad], fill[:, :pad]) and torch.equal(dst[:, cols[3] :], fill[:, cols[3] :]), "the margins of the destination are untouched"


# ----------------------------------------------------------------------------------------------------------------- persistent walks
def _device_case(B, S, Hq, Hkv, D, masked, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda h: torch.randn(B * S, h * D, device="cuda", generator=g).to(BF16)
    q, k, v, do = rn(Hq), rn(Hkv), rn(Hkv), rn(Hq)
    km = None
    if masked:  # ``right`` on every third sample
        km = torch.ones(B, S, dtype=torch.uint8, device="cuda")
        km[0::3, S - S // 3 :] = 0
    return q, k, v, do, km


def _persistent_case(K, B, Hq, Hkv, D, S, causal, form, masked):
    q, k, v, do, km = _device_case(B, S, Hq, Hkv, D, masked, seed=S + D + B)
    o, lse = K.attn_fwd(q, k, v, B, S, Hq, Hkv, D, key_mask=km, causal=causal)
    full = _nan(q), _nan(k), _nan(v)
    _backward(K, form, q, k, v, o, do, lse, B, S, Hq, Hkv, D, *full, km, causal)
    assert all(bool(torch.isfinite(t.float()).all()) for t in full)
    # batch slices small enough for one workgroup per block in both passes
    step = 511 // Hq
    assert B * Hq >= 512 and step * Hq < 512 and step * Hkv < 512
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        rows = slice(b0 * S, b1 * S)
        part = _nan(q[rows]), _nan(k[rows]), _nan(v[rows])
        _backward(K, form, q[rows], k[rows], v[rows], o[rows], do[rows], lse[b0:b1], b1 - b0, S, Hq, Hkv, D, *part, None if km is None else km[b0:b1], causal)
        for name, a, b in zip(("dq", "dk", "dv"), part, full):
            assert torch.equal(a, b[rows]), f"{name} of samples {b0}..{b1 - 1} differs between the persistent walk and one workgroup per block"
    # the first and the last two samples against fp64
    idx = [0, 1, B - 2, B - 1]
    pick = lambda t, H: torch.stack([A.from_tokens(t[b * S : (b + 1) * S].cpu(), 1, S, H, D)[0] for b in idx])
    ops4 = (pick(q, Hq), pick(k, Hkv), pick(v, Hkv), pick(do, Hq))
    km4 = None if km is None else km[idx].cpu()
    exact = A.reference(*ops4, km4, causal, torch.float64)
    floor = A.reference(*ops4, km4, causal)
    got = {"o": pick(o, Hq), "dq": pick(full[0], Hq), "dk": pick(full[1], Hkv), "dv": pick(full[2], Hkv)}
    label = f"persistent B{B}-S{S}-H{Hq}x{Hkv}-D{D}-{'causal' if causal else 'full'} {form}"
    _check(label, got, exact, floor, km4, causal, ops4, 2 * A.n_blocks(4, Hq, S) + 2 * A.n_blocks(4, Hkv, S))
    fails = A.judge_lse(lse[idx].cpu(), ops4[0], ops4[1], km4, causal)[2]
    assert not fails, fails


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("S", [129, 257, 385])
@pytest.mark.parametrize("D,form", [(64, "recompute"), (128, "spill"), (128, "recompute")])
@pytest.mark.parametrize("B", [128, 64], ids=["both-passes", "dq-pass"])
def test_attention_backward_persistent_walk_at_small_s(K, B, D, form, S, causal):
    """B * Hq >= 512 (and, at B = 128, B * Hkv >= 512): one workgroup walks all blocks of its (sample, head) pair.  The gradients are the bits of the
    runs over batch slices that take one workgroup per block, and the first and last two samples pass the fp64 judgement."""
    _persistent_case(K, B, 8, 4, D, S, causal, form, masked=True)


def test_attention_backward_persistent_walk_at_the_vit_b_training_shape(K):
    """12 heads of 64, S = 197, no mask, B * H = 516 >= 512: ViT-B training's shape class."""
    _persistent_case(K, 43, 12, 12, 64, 197, False, "recompute", masked=False)


# ----------------------------------------------------------------------------------------------------------------- left padding in the backward
@pytest.mark.parametrize("D,form", [(64, "recompute"), (128, "spill"), (128, "recompute")])
@pytest.mark.parametrize("S", [70, 200])
def test_attention_backward_left_padding(K, S, D, form):
    """The backward treats a fully-masked row as contributing nothing.  This equals the reference wherever dO is zero on such rows (a): all three
    gradients pass.  Otherwise dV lacks (1/S) * sum of dO of those rows (b): dq and dk pass, dv passes once that term is added to the kernel's dv,
    and fails without it -- the deviation is pinned, not hidden."""
    B, Hq, Hkv, causal = 2, 4, 2, True
    ops4 = list(A.operands(B, S, Hq, Hkv, D, seed=S + D))
    km = A.key_mask("left", B, S)
    dead = A.fully_masked_rows(B, S, km, causal)
    assert int(dead.sum()) == S // 3
    blocks = A.n_blocks(B, Hq, S) + 2 * A.n_blocks(B, Hkv, S)
    shape = (B, S, Hq, Hkv, D)
    # (a)
    ops_a = ops4[:3] + [ops4[3].masked_fill(dead[:, None, :, None], 0.0)]
    g = _grads(K, form, _forward(K, ops_a, km, causal), shape, causal)
    _check(f"left padding S{S} D{D} {form} (a)", g, A.reference(*ops_a, km, causal, torch.float64), A.reference(*ops_a, km, causal), km, causal, ops_a, blocks)
    # (b)
    exact, floor = A.reference(*ops4, km, causal, torch.float64), A.reference(*ops4, km, causal)
    g = _grads(K, form, _forward(K, ops4, km, causal), shape, causal)
    assert A.judge({"dv": g["dv"]}, exact, floor, km, causal, ops4)[3], "dv without the uniform term must miss the reference"
    print(f"[attention sweep] left padding S{S} D{D} {form} (b): dv rel l2 {A.rel_l2(g['dv'], exact['dv']):.3e} without the uniform term")
    g["dv"] = g["dv"].double() + A.uniform_dv_term(ops4[3], km, causal, Hkv)
    _check(f"left padding S{S} D{D} {form} (b)", g, exact, floor, km, causal, ops4, blocks)
