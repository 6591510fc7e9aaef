"""The decode kernels of csrc/decode.hip on a real MI355X against fp64 and against plain Python (tests/decode_sweep.py): attention at every chunk,
round and key-group edge of all four head dims, per (sample, head) and element by element, on strided caches poisoned with NaN wherever the kernel
has no business reading; needles that pin every key position to its own value row bit for bit; the fused QKV launch at the write positions the
append test leaves out; gemv / gemv_pro at ragged N, partial K trips, every M and strided operands; argmax, cache append and the step's bookkeeping
at their edges.  Every attention case prints its measured c."""

import pytest
import torch

import decode_sweep as S

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN = float("nan")


@pytest.fixture(scope="module")
def O():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import ops_decode

    return ops_decode


@pytest.fixture(scope="module")
def tally():
    return {"judged": 0, "expected": 0, "cases": 0, "c": [], "worst": 0.0}


def _attend(O, ns, splits):
    q, kc, vc, km = S.views(ns, "cuda")
    len_dev = None if ns.len_dev is None else torch.tensor([ns.len_dev], dtype=torch.int32, device="cuda")
    return O.attn_decode(q, kc, vc, ns.host_len, ns.Hq, ns.Hkv, ns.D, key_mask=km, scale=ns.scale, len_dev=len_dev, splits=splits)


# ----------------------------------------------------------------------------------------------------------------- 1. attention against fp64
@pytest.mark.parametrize("case", S.grid_cases() + S.peaked_cases(), ids=lambda c: c.name)
def test_attn_decode_matches_fp64_per_sample_and_head(O, case, tally):
    ns, ex = S.build(case), S.exact(case)
    judged, fails, worst = S.judge(_attend(O, ns, case.splits), ex, case.name)
    S.report(case.name, ex, worst)
    assert ex.c_raw <= S.C_CAP
    assert not fails, "\n".join(fails)
    assert judged == ns.B * ns.Hq, "no (sample, head) is left out of the judgement"
    tally["judged"] += judged
    tally["expected"] += ns.B * ns.Hq
    tally["cases"] += 1
    tally["c"].append(ex.c)
    tally["worst"] = max(tally["worst"], worst)


def test_zz_every_sample_and_head_of_the_grid_was_judged(tally):
    if tally["cases"] != len(S.grid_cases()) + len(S.peaked_cases()):
        pytest.skip("needs the grid to have run")
    print(f"[decode sweep] {tally['cases']} cases, {tally['judged']} (sample, head) pairs judged, c {min(tally['c']):.3e} .. {max(tally['c']):.3e}, "
          f"largest error / bound {tally['worst']:.3f}")
    assert tally["judged"] == tally["expected"] == sum(S.BATCH * c.Hq for c in S.grid_cases() + S.peaked_cases())


# ----------------------------------------------------------------------------------------------------------------- 2. needles
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("D", list(S.GEOMETRY))
def test_every_key_position_reaches_its_own_value_row(O, D, splits):
    ns = S.build_needles(D)
    got = _attend(O, ns, splits).cpu()
    wrong = [f"needle at key {j} (sample {b}): {S.place(D, j, splits)}" for b, j in enumerate(ns.pos) if not S.same_bits(got[b], ns.want[b])]
    assert not wrong, "the context is not the needle's value row bit for bit:\n" + "\n".join(wrong)


# ----------------------------------------------------------------------------------------------------------------- 3. the fused QKV launch
QKV_POSITIONS = [(64, wp) for wp in (0, 63, 64, 511, 512, 1030)] + [(128, wp) for wp in (31, 32, 255, 256, 600)]


@pytest.mark.parametrize("D,wp,group", [(D, wp, (1, 2, 4)[i % 3]) for i, (D, wp) in enumerate(QKV_POSITIONS)])
def test_attn_decode_qkv_equals_the_three_launches_at_every_write_position(O, D, wp, group):
    """append (len = wp + 1), middle overwrite (len = wp + 5: the stale row at wp holds NaN and must not be read), not yet visible (len = wp)."""
    from llm_quest_amd import kernels as KK

    B, Hkv = 2, 2
    Hq = Hkv * group
    cap = wp + 9
    g = torch.Generator().manual_seed(D + wp)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    qkv = rn(B, (Hq + 2 * Hkv) * D).to(BF16).cuda()
    qw, kw = (1 + 0.2 * rn(D)).to(BF16).cuda(), (1 + 0.2 * rn(D)).to(BF16).cuda()
    ang = torch.arange(2048).float()[:, None] * torch.logspace(0, -3, D // 2)[None, :]
    cos, sin = torch.cat([ang.cos(), ang.cos()], 1).cuda().contiguous(), torch.cat([ang.sin(), ang.sin()], 1).cuda().contiguous()
    pos = torch.randint(0, 2048, (B,), generator=g, dtype=torch.int32).cuda()
    write_pos = torch.tensor([wp], dtype=torch.int32, device="cuda")
    k_fill, v_fill = rn(B, cap, Hkv * D).to(BF16), rn(B, cap, Hkv * D).to(BF16)
    q_ref, k_ref, _ = KK.qknorm_rope_fwd(qkv, qw, kw, cos, sin, pos, Hq, Hkv, D)
    others = [j for j in range(cap) if j != wp]
    for name, n_keys in (("append", wp + 1), ("middle", wp + 5), ("hidden", wp)):
        if n_keys < 1:
            continue
        kc0, vc0 = k_fill.clone(), v_fill.clone()
        for c in (kc0, vc0):
            c[:, n_keys:] = NAN
            c[:, wp] = NAN
        kc0, vc0 = kc0.cuda(), vc0.cuda()
        length = torch.tensor([n_keys], dtype=torch.int32, device="cuda")
        for splits in (1, 3):
            label = f"{name}, splits {splits}"
            kc1, vc1 = kc0.clone(), vc0.clone()
            O.kv_append_dev(k_ref, qkv[:, (Hq + Hkv) * D :], kc1, vc1, write_pos)
            o_ref = O.attn_decode(q_ref, kc1, vc1, cap, Hq, Hkv, D, len_dev=length, splits=splits)
            kc2, vc2 = kc0.clone(), vc0.clone()
            o = O.attn_decode_qkv(qkv, qw, kw, cos, sin, pos, Hq, Hkv, D, kc2, vc2, write_pos, length, splits=splits)
            assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(o_ref.float()).all()), label
            assert S.same_bits(o, o_ref), label
            assert S.same_bits(kc2, kc1) and S.same_bits(vc2, vc1), label
            assert S.same_bits(kc2[:, others], kc0[:, others]) and S.same_bits(vc2[:, others], vc0[:, others]), label
            assert bool(torch.isfinite(kc2[:, wp].float()).all()) and S.same_bits(vc2[:, wp], qkv[:, (Hq + Hkv) * D :]), label


# ----------------------------------------------------------------------------------------------------------------- 4. gemv, gemv_pro
@pytest.mark.parametrize("N,K", S.GEMV_SHAPES)
def test_gemv_matches_fp64_element_by_element(O, N, K):
    ns = S.gemv_case(N, K)
    w = S.nan_framed(ns.w, 8, 8)[0].cuda()[:, 8 : 8 + K]
    worst = 0.0
    for M in range(1, 9):
        x = S.nan_framed(ns.x[:M], 8, 8)[0].cuda()[:, 8 : 8 + K]
        r = S.nan_framed(ns.r[:M], 1, 2)[0].cuda()[:, 1 : 1 + N]
        assert x.stride(0) == K + 16 and w.stride(0) == K + 16 and r.stride(0) == N + 3
        for residual in (False, True):
            ex = S.gemv_exact(ns, M, residual)
            assert ex.c_raw <= S.C_CAP
            worst = max(worst, ex.c)
            y = O.gemv(x, w, residual=r if residual else None)
            fails = S.judge_gemv(y, ex, f"gemv M{M} N{N} K{K} residual {int(residual)}")
            assert y.shape == (M, N) and not fails, fails
    print(f"[decode sweep] gemv N{N} K{K}: largest c {worst:.3e}")


@pytest.mark.parametrize("M,N,K", S.GEMV_PRO_SHAPES)
def test_gemv_pro_equals_the_two_launches_bit_for_bit(O, M, N, K):
    from llm_quest_amd import kernels as KK

    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = (torch.randn(M, K, generator=g) * 3).to(BF16)
    gu = torch.randn(M, 2 * K, generator=g).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16).cuda()
    r = torch.randn(M, N, generator=g).to(BF16).cuda()
    x_view = S.nan_framed(x, 8, 8)[0].cuda()[:, 8 : 8 + K]
    gu_view = S.nan_framed(gu, 8, 16)[0].cuda()[:, 8 : 8 + 2 * K]  # row pitch 2K + 24 > 2K, NaN in the slack
    assert gu_view.stride(0) > 2 * K
    xn, _ = KK.rmsnorm_fwd(x.cuda(), nw, want_rstd=False)
    act = KK.swiglu_fwd(gu.cuda(), K)
    for res in (None, r):
        for got, want in ((O.gemv_pro(x_view, w, "rmsnorm", nw, residual=res), O.gemv(xn, w, residual=res)),
                          (O.gemv_pro(gu_view, w, "swiglu", residual=res), O.gemv(act, w, residual=res))):
            assert got.shape == (M, N) and bool(torch.isfinite(got.float()).all()) and S.same_bits(got, want)


# ----------------------------------------------------------------------------------------------------------------- 5. argmax, append, advance
def _check_argmax(got, want, names, V, label):
    bad = [f"{label}: row {i} ({names[i]}): got {g}, want {'an index of the row' if w == S.IN_RANGE else w}"
           for i, (g, w) in enumerate(zip(got, want)) if not ((0 <= g < V) if w == S.IN_RANGE else g == w)]
    assert not bad, "\n".join(bad[:8])


@pytest.mark.parametrize("V", S.ARGMAX_V)
def test_argmax_rows_at_the_range_wave_and_value_edges(O, V):
    x, want, names, first = S.argmax_case(V)
    idx = [i % x.shape[0] for i in range(300)]
    wide = torch.full((300, V + 5), float("inf"), dtype=BF16)  # the slack of the strided view holds +inf: it must be ignored
    wide[:, :V] = x[idx]
    wide = wide.cuda()
    for label, logits in (("300 rows, pitch V + 5", wide[:, :V]), ("300 rows, dense", wide[:, :V].contiguous())):
        _check_argmax(O.argmax_rows(logits).tolist(), [want[i] for i in idx], [names[i] for i in idx], V, label)
    for i in first:  # one row per launch, one launch per kind of pattern
        _check_argmax(O.argmax_rows(wide[i : i + 1, :V]).tolist(), [want[i]], [names[i]], V, "1 row")


def test_kv_append_writes_one_row_and_nothing_else(O):
    B, width, cap = 3, 8 * 87, 6
    ld, rows_ld = width + 8, 2 * width + 24
    assert (B * width // 8) % 256 != 0
    g = torch.Generator().manual_seed(4)
    rows = torch.randn(B, rows_ld, generator=g).to(BF16).cuda()
    k_rows, v_rows = rows[:, 8 : 8 + width], rows[:, 16 + width : 16 + 2 * width]
    ks, vs = torch.randn(B * (cap + 3) * ld, generator=g).to(BF16).cuda(), torch.randn(B * (cap + 3) * ld, generator=g).to(BF16).cuda()
    for p in (0, cap - 1, cap, -1):
        k_got, v_got, k_want, v_want = ks.clone(), vs.clone(), ks.clone(), vs.clone()
        O.kv_append_dev(k_rows, v_rows, S.cache_view(k_got, B, cap, width, ld), S.cache_view(v_got, B, cap, width, ld), torch.tensor([p], dtype=torch.int32, device="cuda"))
        if 0 <= p < cap:
            S.cache_view(k_want, B, cap, width, ld)[:, p] = k_rows
            S.cache_view(v_want, B, cap, width, ld)[:, p] = v_rows
            assert not S.same_bits(k_want, ks)
        assert S.same_bits(k_got, k_want) and S.same_bits(v_got, v_want), f"position {p}: the whole storage, slack and other rows included"


@pytest.mark.parametrize("B", [65, 130])
def test_decode_advance_with_several_blocks_moves_the_scalars_once(O, B):
    nxt = torch.arange(B, device="cuda") * 3 + 7
    tok = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
    rope = (torch.arange(B, dtype=torch.int32) * 2 + 1).cuda()
    wp, ln = torch.tensor([10], dtype=torch.int32, device="cuda"), torch.tensor([11], dtype=torch.int32, device="cuda")
    O.decode_advance(nxt, tok, rope, wp, ln)
    assert tok.view(-1).tolist() == [3 * i + 7 for i in range(B)] and rope.tolist() == [2 * i + 2 for i in range(B)]
    assert wp.item() == 11 and ln.item() == 12
