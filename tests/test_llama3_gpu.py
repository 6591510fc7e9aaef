"""The Llama 3.2 / QK-Clip kernels (csrc/llama3.hip), ``Llama3Model`` and ``common/qk_clip.py`` on the GPU, against the plain-torch restatement
(tests/llama3_oracle.py) and the reference fixture (tests/golden/llama3_tiny*.safetensors).

Tolerance: the project's 1.5x rule -- the relative L2 distance of a kernel output to the fp64 restatement is at most 1.5 x the
distance of the reference-dtype-flow restatement to the same fp64 result, with 2e-3 absolute slack only where that floor is below 1e-2.  Each kernel
is judged on the reference flow's operands, so that it answers for its own arithmetic.  The fused RoPE is held to ``kernels.rope_apply`` bit for bit.
"""

import pytest
import torch

import llama3_oracle as LO

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
CFG = LO.TINY_LLAMA
NEG_INF = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _kl():
    from llm_quest_amd import kernels_llama as KL

    return KL


def judge(name, mine, ref_flow, exact, report):
    mine, ref_flow, exact = mine.detach().cpu(), ref_flow.detach().cpu(), exact.detach().cpu()
    assert mine.shape == exact.shape, (name, mine.shape, exact.shape)
    floor = LO.rel_l2(ref_flow, exact)
    got = LO.rel_l2(mine, exact)
    bound = 1.5 * floor + (0.0 if floor >= 1e-2 else 2e-3)
    print(f"  {name}: kernel {got:.3e}  reference flow {floor:.3e}  bound {bound:.3e}")
    if not got <= bound:
        report.append(f"{name}: {got:.3e} > {bound:.3e} (floor {floor:.3e})")


# ----------------------------------------------------------------------------------------------------------------- fused RoPE
ROPE_SHAPES = [(1, 2, 1, 64, False), (70, 4, 2, 64, False), (129, 2, 2, 128, False), (600, 8, 2, 64, False), (70, 4, 2, 64, True)]


@pytest.mark.parametrize("M,Hq,Hkv,D,strided", ROPE_SHAPES)
def test_fused_rope_is_rope_apply_bit_for_bit(M, Hq, Hkv, D, strided):
    """Forward and adjoint against ``kernels.rope_apply`` on the same operands, positions shuffled (non-monotonic); one case on a row-strided qkv."""
    from llm_quest_amd import kernels as K

    KL = _kl()
    g = torch.Generator().manual_seed(M * 7 + Hq)
    W = (Hq + 2 * Hkv) * D
    ctx = M + 5
    cos, sin = (t.cuda() for t in LO.rope_tables(500_000, D, ctx))
    pos = torch.randperm(ctx, generator=g)[:M].to(torch.int32).cuda()
    buf = torch.randn(M, W + (64 if strided else 0), generator=g).to(BF16).cuda()
    qkv = buf[:, :W]
    assert qkv.is_contiguous() != strided or M == 1
    q, k = KL.rope_fwd(qkv, cos, sin, pos, Hq, Hkv, D)
    heads = lambda t, H: t.reshape(1, M, H, D).transpose(1, 2)  # (1, H, M, D) view of token-major rows
    back = lambda t, H: t.transpose(1, 2).reshape(M, H * D)
    want_q = back(K.rope_apply(heads(qkv[:, : Hq * D], Hq), cos, sin, pos), Hq)
    want_k = back(K.rope_apply(heads(qkv[:, Hq * D : (Hq + Hkv) * D], Hkv), cos, sin, pos), Hkv)
    assert q.shape == (M, Hq * D) and k.shape == (M, Hkv * D) and q.is_contiguous() and k.is_contiguous()
    assert torch.equal(q, want_q) and torch.equal(k, want_k)
    # and against the restatement, which is exact about every rounding too
    oq, ok = LO.rope_packed_fwd(qkv.cpu(), cos.cpu(), sin.cpu(), pos.cpu(), 1, M, Hq, Hkv, D)
    assert torch.equal(q.cpu(), oq) and torch.equal(k.cpu(), ok)

    dq = torch.randn(M, Hq * D, generator=g).to(BF16).cuda()
    dk = torch.randn(M, Hkv * D, generator=g).to(BF16).cuda()
    dbuf = torch.full((M, W + (64 if strided else 0)), 7.0, dtype=BF16, device="cuda")
    dqkv = dbuf[:, :W]
    KL.rope_bwd(dq, dk, cos, sin, pos, dqkv, Hq, Hkv, D)
    want_dq = back(K.rope_apply(heads(dq, Hq), cos, sin, pos, transpose=True), Hq)
    want_dk = back(K.rope_apply(heads(dk, Hkv), cos, sin, pos, transpose=True), Hkv)
    assert torch.equal(dqkv[:, : Hq * D], want_dq) and torch.equal(dqkv[:, Hq * D : (Hq + Hkv) * D], want_dk)
    assert bool((dbuf[:, (Hq + Hkv) * D :] == 7.0).all())  # the v columns (and what lies behind the row) are the caller's


def test_fused_rope_refuses_bad_operands():
    KL = _kl()
    cos, sin = (t.cuda() for t in LO.rope_tables(10_000, 64, 16))
    pos = torch.arange(8, dtype=torch.int32, device="cuda")
    qkv = torch.zeros(8, 256, dtype=BF16, device="cuda")
    with pytest.raises(ValueError, match="not built"):
        KL.rope_fwd(qkv, cos, sin, pos, 4, 2, 32)
    with pytest.raises(ValueError, match="multiple of kv heads"):
        KL.rope_fwd(qkv, cos, sin, pos, 3, 2, 64)
    with pytest.raises(ValueError, match="unit inner stride"):
        KL.rope_fwd(qkv.float(), cos, sin, pos, 2, 1, 64)
    with pytest.raises(ValueError, match="pos must be"):
        KL.rope_fwd(qkv, cos, sin, pos.long(), 2, 1, 64)
    with pytest.raises(ValueError, match="contiguous fp32"):
        KL.rope_fwd(qkv, cos.to(BF16), sin, pos, 2, 1, 64)


# ----------------------------------------------------------------------------------------------------------------- maximum attention logit
# (B, S, Hq, Hkv, D): the issue's five, then the kernel's own edges: one key tile exactly and one key past it, one 128-query block exactly, and three
# blocks of three samples (nine partials per head)
MAX_SHAPES = [(1, 1, 2, 1, 64), (2, 31, 4, 2, 64), (2, 70, 4, 2, 64), (1, 129, 2, 2, 128), (2, 300, 8, 2, 64),
              (1, 32, 2, 1, 128), (1, 33, 2, 1, 64), (1, 128, 2, 1, 64), (3, 257, 2, 2, 64)]
MASKS = ("none", "right", "left")


def _mask(kind, B, S):
    """bool [B, S] or None; at least one key of every sample stays on."""
    if kind == "none":
        return None
    m = torch.ones(B, S, dtype=torch.bool)
    for b in range(B):
        pad = min(S - 1, (3, max(S // 3, 1))[b % 2])
        if pad:
            if kind == "right":
                m[b, S - pad :] = False
            else:
                m[b, :pad] = False
    return m


def _run_max(q, k, mask, scale=None):
    """The kernel on [B, H, S, D] CPU operands -> fp32 [Hq] on the CPU."""
    KL = _kl()
    B, Hq, S, D = q.shape
    km = None if mask is None else mask.to(torch.uint8).cuda()
    return KL.attn_max_logit(LO.to_tokens(q).cuda(), LO.to_tokens(k).cuda(), B, S, Hq, k.shape[1], D, key_mask=km, scale=scale).cpu()


@pytest.mark.parametrize("B,S,Hq,Hkv,D", MAX_SHAPES)
def test_max_logit_against_fp64(B, S, Hq, Hkv, D):
    report = []
    q, k = LO.attn_operands(B, S, Hq, Hkv, D, seed=S * 13 + D)
    for kind in MASKS:
        mask = _mask(kind, B, S)
        got = _run_max(q, k, mask)
        assert got.dtype == F32 and got.shape == (Hq,)
        judge(f"max_logit {kind}", got, LO.max_logit(q, k, key_mask=mask), LO.max_logit(q, k, key_mask=mask, exact=True), report)
    assert not report, "\n".join(report)


def _plant(q, k, h, b, i, j, a, half):
    """q[b, h, i] = k[b, g, j] = a on one half of the features, 0 on the other: a logit of scale * a^2 * D / 2, and no product with a plant on the
    other half."""
    D = q.shape[-1]
    g = h // (q.shape[1] // k.shape[1])
    e = torch.zeros(D)
    e[: D // 2] = 1.0
    if half:
        e = 1.0 - e
    q[b, h, i] = (a * e).to(BF16)
    k[b, g, j] = (a * e).to(BF16)


def _argmax_visible(q, k, mask, h):
    """(b, i, j) of the largest visible fp64 logit of head h."""
    s = LO.scores(q, k, exact=True)
    B, _, S, _ = s.shape
    s = torch.where(LO.visible(B, S, mask), s, torch.full((), NEG_INF, dtype=s.dtype))[:, h]
    flat = int(s.reshape(-1).argmax())
    return flat // (S * S), (flat // S) % S, flat % S


@pytest.mark.parametrize("B,S,Hq,Hkv,D", MAX_SHAPES)
def test_max_logit_finds_planted_maxima_and_ignores_invisible_ones(B, S, Hq, Hkv, D):
    """One visible plant per run -- on the diagonal, at (S - 1, 0), in the last ragged key tile, in the last sample only, on a padded query row that
    still sees real keys -- is reported exactly (its operands are small integers); a strictly larger plant at an invisible pair (the key right of the
    diagonal, or a masked key) changes nothing.  The fp64 visible maximum is checked to sit at the visible plant first."""
    h = Hq - 1
    last_tile = ((S - 1) // 32) * 32
    plants = {"diagonal": ("none", 0, S // 2, S // 2), "corner": ("none", 0, S - 1, 0), "last tile": ("left", 0, S - 1, last_tile),
              "last sample": ("right", B - 1, S // 2, S // 2 if S < 4 else S // 4), "padded query": ("right", 0, S - 1, 0)}
    checked_invisible = 0
    for name, (kind, b, i, j) in plants.items():
        mask = _mask(kind, B, S)
        if mask is not None and not bool(mask[b, j]):
            j = int(mask[b].nonzero()[0 if j < S // 2 else -1])  # the plant's key must be a real one
            i = max(i, j)
        q, k = LO.attn_operands(B, S, Hq, Hkv, D, seed=S + 17 * len(name))
        _plant(q, k, h, b, i, j, 2.0, half=0)
        want = (D ** -0.5) * 4.0 * (D // 2)
        assert _argmax_visible(q, k, mask, h) == (b, i, j), name
        exact = LO.max_logit(q, k, key_mask=mask, exact=True)
        assert float(exact[h]) == pytest.approx(want, rel=1e-12)
        got = _run_max(q, k, mask)
        assert float(got[h]) == float(torch.tensor(float(exact[h]), dtype=F32)), (name, float(got[h]), want)
        if name == "padded query" and S > 1:
            assert not bool(mask[b, i]) and bool(mask[b, j])  # the query row is padding, its key is not
        # strictly larger plants at invisible pairs
        for variant in ("right of the diagonal", "masked key"):
            q2, k2 = q.clone(), k.clone()
            if variant == "right of the diagonal":
                if S < 2:
                    continue
                iu = min(S // 3, S - 2)
                b2, ju, mask2 = (b + 1) % B, iu + 1, mask
            else:
                mask2 = _mask("right", B, S) if mask is None else mask
                b2 = (b + 1) % B
                off = (~mask2[b2]).nonzero()
                if off.numel() == 0:
                    continue
                iu, ju = S - 1, int(off[-1])
                if mask2 is not mask and _argmax_visible(q, k, mask2, h) != (b, i, j):
                    continue  # the visible plant must survive the change of mask
            if (b2, iu) == (b, i) or (b2, ju) == (b, j):
                continue  # would overwrite the visible plant's own rows
            _plant(q2, k2, h, b2, iu, ju, 3.0, half=1)
            assert float(LO.scores(q2, k2, exact=True)[b2, h, iu, ju]) > want  # strictly larger, and invisible:
            assert not bool(LO.visible(B, S, mask2)[b2, 0, iu, ju])
            assert _argmax_visible(q2, k2, mask2, h) == (b, i, j), (name, variant)
            got2 = _run_max(q2, k2, mask2)
            assert float(got2[h]) == float(got[h]), (name, variant, float(got2[h]))
            checked_invisible += 1
    assert checked_invisible >= (2 if S > 1 else 0)


def _int_operands(B, S, Hq, Hkv, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-2, 3, (B, Hq, S, D), generator=g).to(BF16), torch.randint(-2, 3, (B, Hkv, S, D), generator=g).to(BF16))


def test_max_logit_is_exact_on_integer_operands():
    """Integers in [-2, 2], D = 64, scale = 0.125: every product, sum and the scaling are exact in fp32, so the result is the fp64 value bit for bit.
    Also: a fully masked sample beside a live one contributes nothing; two runs give the same bits."""
    B, S, Hq, Hkv, D = 2, 70, 4, 2, 64
    q, k = _int_operands(B, S, Hq, Hkv, D, 5)
    for kind in MASKS:
        mask = _mask(kind, B, S)
        got = _run_max(q, k, mask, scale=0.125)
        exact = LO.max_logit(q, k, 0.125, mask, exact=True)
        assert torch.equal(got.double(), exact), kind
        assert torch.equal(got, _run_max(q, k, mask, scale=0.125))
    mask = torch.ones(B, S, dtype=torch.bool)
    mask[0] = False
    got = _run_max(q, k, mask, scale=0.125)
    assert torch.equal(got.double(), LO.max_logit(q[1:], k[1:], 0.125, None, exact=True))
    assert torch.equal(got.double(), LO.max_logit(q, k, 0.125, mask, exact=True))


def test_max_logit_without_a_visible_pair_is_minus_infinity():
    KL = _kl()
    B, S, Hq, Hkv, D = 2, 40, 4, 2, 64
    q, k = _int_operands(B, S, Hq, Hkv, D, 6)
    got = _run_max(q, k, torch.zeros(B, S, dtype=torch.bool))
    assert got.tolist() == [NEG_INF] * Hq
    assert LO.max_logit(q, k, key_mask=torch.zeros(B, S, dtype=torch.bool), exact=True).tolist() == [NEG_INF] * Hq
    # an empty problem has no pair either
    z = torch.zeros(0, Hq * D, dtype=BF16, device="cuda")
    assert KL.attn_max_logit(z, z[:, : Hkv * D], 0, 5, Hq, Hkv, D).tolist() == [NEG_INF] * Hq
    # only the first key is real: every row sees exactly that key
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[:, 0] = True
    assert torch.equal(_run_max(q, k, mask, 0.125).double(), LO.max_logit(q, k, 0.125, mask, exact=True))


def test_max_logit_propagates_nan_to_its_head_only():
    B, S, Hq, Hkv, D = 2, 70, 4, 2, 64
    q, k = _int_operands(B, S, Hq, Hkv, D, 7)
    clean = _run_max(q, k, None, 0.125)
    q2 = q.clone()
    q2[1, 1, 37, 5] = float("nan")
    got = _run_max(q2, k, None, 0.125)
    assert bool(torch.isnan(got[1])) and torch.equal(got[[0, 2, 3]], clean[[0, 2, 3]])
    want = LO.max_logit(q2, k, 0.125, None, exact=True)
    assert bool(torch.isnan(want[1])) and torch.equal(want[[0, 2, 3]], clean[[0, 2, 3]].double())
    # a NaN on a key nobody sees (masked) is not reported
    mask = torch.ones(B, S, dtype=torch.bool)
    mask[0, 69] = False
    k2 = k.clone()
    k2[0, 0, 69] = float("nan")
    got = _run_max(q, k2, mask, 0.125)
    assert not bool(torch.isnan(got).any()) and torch.equal(got.double(), LO.max_logit(q, k2, 0.125, mask, exact=True))


def test_max_logit_takes_row_strided_operands_and_refuses_bad_ones():
    KL = _kl()
    B, S, Hq, Hkv, D = 2, 70, 4, 2, 64
    q, k = _int_operands(B, S, Hq, Hkv, D, 8)
    packed = torch.cat((LO.to_tokens(q), LO.to_tokens(k)), dim=1).cuda()  # q | k as column slices of one matrix
    got = KL.attn_max_logit(packed[:, : Hq * D], packed[:, Hq * D :], B, S, Hq, Hkv, D, scale=0.125)
    assert torch.equal(got.cpu().double(), LO.max_logit(q, k, 0.125, None, exact=True))
    qt, kt = LO.to_tokens(q).cuda(), LO.to_tokens(k).cuda()
    with pytest.raises(ValueError, match="not built"):
        KL.attn_max_logit(qt, kt, B, S, Hq * 2, Hkv * 2, 32)
    with pytest.raises(ValueError, match="multiple of kv heads"):
        KL.attn_max_logit(qt, kt, B, S, Hq, 3, D)
    with pytest.raises(ValueError, match="key_mask"):
        KL.attn_max_logit(qt, kt, B, S, Hq, Hkv, D, key_mask=torch.ones(B, S, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="tokens="):
        KL.attn_max_logit(qt[:-1], kt, B, S, Hq, Hkv, D)


# ----------------------------------------------------------------------------------------------------------------- QK-Clip
TAU = 4.0
NAN = float("nan")
# (Hq, Hkv, D, d_in, maxima): a head at exactly tau, one at -inf, one NaN; in the first two only ONE query head of a group exceeds tau
CLIP_CASES = [(4, 2, 64, 256, [TAU, 16.0, NAN, NEG_INF]), (8, 2, 128, 1024, [1.0, 5.0, 2.0, 3.0, TAU, NAN, NEG_INF, -2.0]), (2, 2, 64, 72, [8.0, TAU])]


def _weights(Hq, Hkv, D, d_in, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Hq * D, d_in, generator=g).to(BF16), torch.randn(Hkv * D, d_in, generator=g).to(BF16)


def _run_clip(wq, wk, m, Hq, Hkv, alpha, mode):
    KL = _kl()
    gq, gk = wq.clone().cuda(), wk.clone().cuda()
    KL.qk_clip_(gq, gk, m.cuda(), Hq, Hkv, TAU, alpha, mode)
    return gq.cpu(), gk.cpu()


def _judge_clip(name, wq, wk, m, Hq, Hkv, alpha, mode, got, report):
    """Untouched heads are the input bit for bit; the clipped ones are judged under the rule against float64(w) * gamma^e, the reference flow being
    upstream's arithmetic (an fp32 product rounded once to bf16), and lie within one bf16 step of it."""
    want = LO.qk_clip(wq, wk, m, Hq, Hkv, TAU, alpha, mode)
    g = LO.clip_gammas(m, TAU, mode).double()
    gk = g.view(Hkv, Hq // Hkv).min(dim=1).values
    for w, mine, ref, gam, e, H, which in ((wq, got[0], want[0], g, alpha, Hq, "wq"), (wk, got[1], want[1], gk, 1 - alpha, Hkv, "wk")):
        w3, m3, r3 = (x.view(H, -1, x.shape[1]) for x in (w, mine, ref))
        for h in range(H):
            if float(gam[h]) >= 1.0:
                if not torch.equal(m3[h], w3[h]):
                    report.append(f"{name} {which} head {h}: written although it does not clip")
            else:
                judge(f"{name} {which} head {h}", m3[h], r3[h], w3[h].double() * float(gam[h]) ** e, report)
        report += [f"{name} {which} {x}" for x in LO.clip_mismatches(w, mine, ref, H)]


@pytest.mark.parametrize("Hq,Hkv,D,d_in,maxima", CLIP_CASES)
@pytest.mark.parametrize("alpha", [0.5, 0.3])
def test_qk_clip_per_head(Hq, Hkv, D, d_in, maxima, alpha):
    report = []
    wq, wk = _weights(Hq, Hkv, D, d_in, Hq + d_in)
    m = torch.tensor(maxima, dtype=F32)
    got = _run_clip(wq, wk, m, Hq, Hkv, alpha, "per_head")
    _judge_clip("per_head", wq, wk, m, Hq, Hkv, alpha, "per_head", got, report)
    clips = [h for h, v in enumerate(maxima) if v > TAU]
    assert len(clips) == 1
    rep = Hq // Hkv
    q3, k3 = got[0].view(Hq, D, d_in), got[1].view(Hkv, D, d_in)
    for h in range(Hq):  # exactly the head above tau, and its group's key head, moved
        assert torch.equal(q3[h], wq.view(Hq, D, d_in)[h]) == (h not in clips), h
    for gidx in range(Hkv):
        assert torch.equal(k3[gidx], wk.view(Hkv, D, d_in)[gidx]) == (gidx != clips[0] // rep), gidx
    assert not report, "\n".join(report)


@pytest.mark.parametrize("Hq,Hkv,D,d_in,maxima", CLIP_CASES)
def test_qk_clip_naive_and_magnitude(Hq, Hkv, D, d_in, maxima):
    KL = _kl()
    report = []
    wq, wk = _weights(Hq, Hkv, D, d_in, Hq + d_in + 1)
    m = torch.tensor(maxima, dtype=F32)
    # naive: a NaN on any head leaves the layer alone; without it the largest head decides for every row of both matrices
    got = _run_clip(wq, wk, m, Hq, Hkv, 0.5, "naive")
    has_nan = bool(torch.isnan(m).any())
    assert (torch.equal(got[0], wq) and torch.equal(got[1], wk)) == has_nan
    m_clean = torch.where(torch.isnan(m), torch.full_like(m, -3.0), m)
    for alpha in (0.5, 0.3):
        got = _run_clip(wq, wk, m_clean, Hq, Hkv, alpha, "naive")
        _judge_clip("naive", wq, wk, m_clean, Hq, Hkv, alpha, "naive", got, report)
        assert not torch.equal(got[0].view(Hq, D, d_in)[0], wq.view(Hq, D, d_in)[0]) and not torch.equal(got[1], wk)
    low = torch.full((Hq,), TAU, dtype=F32)
    got = _run_clip(wq, wk, low, Hq, Hkv, 0.5, "naive")
    assert torch.equal(got[0], wq) and torch.equal(got[1], wk)
    # magnitude: multi-head attention only; a large negative maximum clips too
    if Hq == Hkv:
        mm = torch.tensor([-8.0, 3.0], dtype=F32)
        got = _run_clip(wq, wk, mm, Hq, Hkv, 0.5, "magnitude")
        _judge_clip("magnitude", wq, wk, mm, Hq, Hkv, 0.5, "magnitude", got, report)
        assert not torch.equal(got[0][:D], wq[:D]) and torch.equal(got[0][D:], wq[D:]) and torch.equal(got[1][D:], wk[D:])
        got = _run_clip(wq, wk, mm, Hq, Hkv, 0.5, "per_head")  # the signed rule leaves both alone
        assert torch.equal(got[0], wq) and torch.equal(got[1], wk)
    else:
        with pytest.raises(ValueError, match="multi-head attention only"):
            KL.qk_clip_(wq.cuda(), wk.cuda(), m.cuda(), Hq, Hkv, TAU, 0.5, "magnitude")
    assert not report, "\n".join(report)


def test_qk_clip_refuses_views_it_cannot_scale_in_place():
    KL = _kl()
    wq, wk = (t.cuda() for t in _weights(4, 2, 64, 256, 3))
    m = torch.zeros(4, device="cuda")
    with pytest.raises(ValueError, match="contiguous bf16"):
        KL.qk_clip_(wq[:, ::2], wk[:, ::2], m, 4, 2, TAU)
    with pytest.raises(ValueError, match="contiguous bf16"):
        KL.qk_clip_(wq.float(), wk, m, 4, 2, TAU)
    with pytest.raises(ValueError, match="max_logits"):
        KL.qk_clip_(wq, wk, m.double(), 4, 2, TAU)
    with pytest.raises(ValueError, match="positive"):
        KL.qk_clip_(wq, wk, m, 4, 2, 0.0)
    # an unaligned (but contiguous) pair takes the element-wise path
    base = torch.randn(4 * 64 * 40 + 2 * 64 * 40 + 1).to(BF16).cuda()
    uq, uk = base[1 : 1 + 4 * 64 * 40].view(256, 40), base[1 + 4 * 64 * 40 :].view(128, 40)
    assert uq.data_ptr() % 16 and uq.is_contiguous()
    before_q, before_k = uq.cpu().clone(), uk.cpu().clone()
    mm = torch.tensor([8.0, 1.0, 1.0, 1.0])
    KL.qk_clip_(uq, uk, mm.cuda(), 4, 2, TAU, 0.5)
    want = LO.qk_clip(before_q, before_k, mm, 4, 2, TAU, 0.5)
    assert not LO.clip_mismatches(before_q, uq, want[0], 4) and not LO.clip_mismatches(before_k, uk, want[1], 2)
    assert not torch.equal(uq.cpu()[:64], before_q[:64])


# ----------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def fixture():
    return LO.load_fixture("llama3_tiny")


@pytest.fixture(scope="module")
def exact_model(fixture):
    """The fp64 restatement on the fixture, computed once: logits with and without the mask and the per-layer maxima."""
    t = fixture
    sd = LO.state_dict_of(t)
    cap = []
    with torch.no_grad():
        logits = LO.model(sd, CFG, t["in.ids"], t["in.key_mask"], exact=True, capture=cap)
        nomask = LO.model(sd, CFG, t["in.ids"], exact=True)
    return dict(logits=logits, nomask=nomask, maxima=cap)


def _model(t, **over):
    from llm_quest_amd.gpt_to_llama3.llama_model import Llama3Model

    m = Llama3Model(dict(CFG, **over)).to(BF16)
    missing, unexpected = m.load_state_dict(LO.state_dict_of(t), strict=False)
    assert not unexpected and set(missing) <= {"mask", "cos", "sin", "out_head.weight"}
    return m.cuda().train()


def _track(m, on=True):
    for blk in m.trf_blocks:
        blk.att.track_max_attn_logit = on


def _step(m, t):
    """One forward + backward of the masked batch: (loss, {name: gradient clone})."""
    ids, tgt, km = t["in.ids"].cuda(), t["in.targets"].cuda(), t["in.key_mask"].bool().cuda()
    m.zero_grad(set_to_none=True)
    h = m.forward_hidden(ids, km)
    loss = m.lm_loss(h.reshape(-1, h.shape[-1]), tgt)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def test_model_against_the_fixture(fixture, exact_model):
    from llm_quest_amd.common.qk_clip import collect_max_attn_logits

    t = fixture
    report = []
    m = _model(t)
    _track(m)
    ids, km = t["in.ids"].cuda(), t["in.key_mask"].bool().cuda()
    with torch.no_grad():
        logits = m(ids, km)
        tracked = [x.clone() for x in collect_max_attn_logits(m)]
        nomask = m(ids)
    assert logits.dtype == BF16 and logits.shape == t["out.logits"].shape
    judge("logits", logits, t["out.logits"], exact_model["logits"], report)
    judge("logits without the mask", nomask, t["out.logits_nomask"], exact_model["nomask"], report)
    for i, got in enumerate(tracked):
        assert got.dtype == F32 and got.shape == (CFG["n_heads"],) and got.is_cuda
        judge(f"max_attn_logit of layer {i}", got, t[f"out.max_logits.{i}"], exact_model["maxima"][i], report)
    loss, grads = _step(m, t)
    print(f"  loss: model {float(loss):.6f}  reference bf16 {float(t['out.loss']):.6f}  fp32 twin {float(t['twin.loss']):.6f}")
    assert loss.dtype == F32 and abs(float(loss) - float(t["twin.loss"])) / float(t["twin.loss"]) < 1e-3
    names = [k[10:] for k in t if k.startswith("twin.grad.")]
    assert set(names) == set(grads) and len(names) == 22
    for n in names:  # every gradient, the reference's own tensor as the floor
        judge("grad " + n, grads[n], t["grad." + n], t["twin.grad." + n], report)
    assert not report, "\n".join(report)


def test_attention_module_on_its_own(fixture):
    """``GroupedQueryAttention.forward`` outside a block (its own autograd node and arena): output, dx and the five parameter gradients under the rule
    against the restatement differentiated in fp64, the restatement in the reference's dtype flow as the floor."""
    t = fixture
    report = []
    m = _model(t)
    att = m.trf_blocks[0].att
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 24, CFG["emb_dim"], generator=g).to(BF16)
    dy = torch.randn(2, 24, CFG["emb_dim"], generator=g).to(BF16)
    km = t["in.key_mask"].bool()
    xg = x.cuda().requires_grad_(True)
    y = att(xg, m.mask, m.cos, m.sin, km.cuda())
    y.backward(dy.cuda())
    pfx = "trf_blocks.0.att."
    sd = {k[len(pfx):]: v for k, v in LO.state_dict_of(t).items() if k.startswith(pfx)}
    cos, sin = LO.tables(CFG)

    def restated(dtype):
        leaves = {k: v.to(dtype).detach().requires_grad_(True) for k, v in sd.items()}
        xr = x.to(dtype).detach().requires_grad_(True)
        yr = LO.gqa(leaves, "", xr, CFG, cos, sin, km)
        grads = torch.autograd.grad(yr, [xr] + list(leaves.values()), dy.to(dtype))
        return yr.detach(), grads[0], dict(zip(leaves, grads[1:]))

    (y_f, dx_f, g_f), (y_e, dx_e, g_e) = restated(BF16), restated(torch.float64)
    judge("attention y", y, y_f, y_e, report)
    judge("attention dx", xg.grad, dx_f, dx_e, report)
    assert set(g_e) == {n for n, _ in att.named_parameters()} and len(g_e) == 5
    for n, p in att.named_parameters():
        judge("attention grad " + n, p.grad, g_f[n], g_e[n], report)
    assert not report, "\n".join(report)


def test_model_is_bit_reproducible_and_tracking_changes_nothing(fixture):
    t = fixture
    ids, km = t["in.ids"].cuda(), t["in.key_mask"].bool().cuda()
    runs = []
    for tracking in (False, False, True):
        m = _model(t)
        _track(m, tracking)
        with torch.no_grad():
            logits = m(ids, km)
        loss, grads = _step(m, t)
        runs.append((logits, loss, grads))
        assert (m.trf_blocks[0].att.max_attn_logit is not None) == tracking
    for other in runs[1:]:
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1])
        for n, g in runs[0][2].items():
            assert torch.equal(g, other[2][n]), n


def test_tracking_off_launches_what_the_block_launches_without_it(fixture):
    """With tracking off no ``mi355_attn_max_logit`` is launched; with it on exactly one per layer and forward, nothing else changes."""
    from llm_quest_amd import _lib as L

    t = fixture
    ids = t["in.ids"].cuda()
    m = _model(t)
    with torch.no_grad():
        m(ids)  # the first forward also casts the RoPE tables back to fp32
    names, real = [], L.call

    def counting(name, *args):
        names.append(name)
        return real(name, *args)

    seen = {}
    L.call = counting
    try:
        for tracking in (False, True):
            _track(m, tracking)
            names.clear()
            with torch.no_grad():
                m(ids)
            seen[tracking] = list(names)
    finally:
        L.call = real
    assert "mi355_attn_max_logit" not in seen[False]
    assert seen[True].count("mi355_attn_max_logit") == CFG["n_layers"]
    assert [n for n in seen[True] if n != "mi355_attn_max_logit"] == seen[False]
    assert seen[False].count("mi355_llama_rope_fwd") == CFG["n_layers"] and seen[False].count("mi355_attn_fwd") == CFG["n_layers"]


def test_fixture_clips_are_reproduced_by_the_kernel(fixture):
    """The reference's QKClip(4.0), QKClipNaive(4.0) and MagnitudeQKClipMHA(4.0) on the fixture's maxima: heads it left alone bit for bit, the
    others within one bf16 step."""
    KL = _kl()
    t = fixture
    Hq, Hkv = CFG["n_heads"], CFG["num_kv_groups"]
    bad = []
    for mode, sdp, mp, cp, hkv in (("per_head", "sd.", "out.max_logits.", "clip.per_head.", Hkv), ("naive", "sd.", "out.max_logits.", "clip.naive.", Hkv),
                                   ("magnitude", "mha.sd.", "mha.max_logits.", "mha.clip.magnitude.", Hq)):
        for i in range(CFG["n_layers"]):
            pq, pk = f"trf_blocks.{i}.att.w_queries.weight", f"trf_blocks.{i}.att.w_keys.weight"
            gq, gk = t[sdp + pq].clone().cuda(), t[sdp + pk].clone().cuda()
            KL.qk_clip_(gq, gk, t[f"{mp}{i}"].cuda(), Hq, hkv, LO.FIXTURE_TAU, 0.5, mode)
            bad += [f"{mode} layer {i} wq {x}" for x in LO.clip_mismatches(t[sdp + pq], gq, t[cp + pq], Hq)]
            bad += [f"{mode} layer {i} wk {x}" for x in LO.clip_mismatches(t[sdp + pk], gk, t[cp + pk], hkv)]
    assert not bad, "\n".join(bad)


def test_clip_and_tracked_forward_do_not_read_the_device(fixture):
    """``QKClip.__call__`` and a tracked forward under torch.cuda.set_sync_debug_mode("error"): neither synchronises with the host."""
    from llm_quest_amd.common.qk_clip import QKClip, QKClipNaive, collect_max_attn_logits

    t = fixture
    m = _model(t)
    _track(m)
    ids, km = t["in.ids"].cuda(), t["in.key_mask"].bool().cuda()
    with torch.no_grad():
        m(ids, km)  # arenas, tables and positions are built here
    probe = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bites = False
        try:
            probe.item()
        except RuntimeError:
            bites = True
        if not bites:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build: the host reads cannot be observed")
        with torch.no_grad():
            m(ids, km)
        maxima = collect_max_attn_logits(m)
        QKClip(LO.FIXTURE_TAU)(m, maxima)
        QKClipNaive(LO.FIXTURE_TAU, alpha=0.3)(m, maxima)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(m.trf_blocks[0].att.w_queries.weight.float()).all())


def test_three_optimizer_steps_with_qk_clip(fixture):
    """ArenaAdamW steps with QKClip(tau) after each, tau the median tracked maximum: after every clip a no-grad forward on the same batch gives
    tracked maxima that agree with the restatement's on the clipped weights under the rule, and the weights of the heads that did not clip are what
    the optimizer left."""
    from llm_quest_amd.common.qk_clip import QKClip, collect_max_attn_logits
    from llm_quest_amd.optim import ArenaAdamW

    t = fixture
    report = []
    Hq, Hkv, D = CFG["n_heads"], CFG["num_kv_groups"], CFG["emb_dim"] // CFG["n_heads"]
    m = _model(t)
    _track(m)
    ids, km = t["in.ids"].cuda(), t["in.key_mask"].bool().cuda()
    with torch.no_grad():
        m(ids, km)
    tau = float(torch.cat(collect_max_attn_logits(m)).median())
    clip = QKClip(tau)
    opt = ArenaAdamW(m.parameters(), lr=1e-3, weight_decay=0.0).attach(m)
    assert len(m.arenas()) == CFG["n_layers"] + 1
    clipped_heads = 0
    for step in range(3):
        _step(m, t)  # zero_grad, tracked forward, backward
        maxima = [x.clone() for x in collect_max_attn_logits(m)]
        opt.step()
        after_opt = [(blk.att.w_queries.weight.detach().clone(), blk.att.w_keys.weight.detach().clone()) for blk in m.trf_blocks]
        clip(m, maxima)
        for i, blk in enumerate(m.trf_blocks):
            over = (maxima[i] > tau).cpu()
            wq, wk = blk.att.w_queries.weight.detach(), blk.att.w_keys.weight.detach()
            for h in range(Hq):  # (a head barely above tau is scaled by less than a bf16 step: it may come out unchanged, so only the heads that moved are counted)
                same = torch.equal(wq[h * D : (h + 1) * D], after_opt[i][0][h * D : (h + 1) * D])
                assert same or bool(over[h]), (step, i, h)
                clipped_heads += not same
            for g in range(Hkv):
                same = torch.equal(wk[g * D : (g + 1) * D], after_opt[i][1][g * D : (g + 1) * D])
                assert same or bool(over.view(Hkv, Hq // Hkv)[g].any()), (step, i, g)
        with torch.no_grad():
            m(ids, km)
        got = [x.cpu() for x in collect_max_attn_logits(m)]
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if k not in ("mask", "cos", "sin", "out_head.weight")}
        flow, exact = [], []
        with torch.no_grad():
            LO.model(sd, CFG, t["in.ids"], t["in.key_mask"], capture=flow)
            LO.model(sd, CFG, t["in.ids"], t["in.key_mask"], exact=True, capture=exact)
        for i in range(CFG["n_layers"]):
            judge(f"step {step} layer {i} post-clip maxima", got[i], flow[i], exact[i], report)
    assert clipped_heads >= 2
    assert not report, "\n".join(report)
