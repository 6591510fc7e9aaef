"""MiMo-V2-Flash kernels (csrc/attention_band.hip, csrc/mimo.hip) and MiMoModel on the GPU, against the plain-torch restatement (tests/mimo_oracle.py) and the reference
fixture (tests/golden/mimo_tiny*.safetensors).

Tolerance: the project's 1.5x rule exactly as tests/test_gemma3_gpu.py's ``judge`` implements it, and nothing else -- the
relative L2 distance of a kernel output to the fp64 restatement is at most 1.5 x the distance of the reference-dtype-flow restatement to the same
fp64 result, with 2e-3 absolute slack only where that floor is below 1e-2; where the fp64 result is identically zero the kernel is held to 1e-6
absolute per element.
"""

import json
import os

import pytest
import torch

import mimo_oracle as O
from test_gemma3_gpu import _check_padded, _padded, judge

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
CFG = O.TINY_MIMO
LAYERS = O.moe_layers(CFG)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _km():
    from llm_quest_amd import kernels_mimo as KM

    return KM


# ----------------------------------------------------------------------------------------------------------------- sink attention
ATTN_CASES = [  # (B, S, Hq, Hkv, D, DV, W, sink)
    (1, 1, 2, 1, 64, 32, 1, True),  # a single token: the key itself and the sink
    (2, 70, 6, 2, 64, 32, 5, True),  # window inside one key tile, ragged S, GQA ratio 3
    (1, 129, 2, 2, 64, 32, 32, True),  # window equal to the tile width, one query past a 128-query block
    (1, 129, 2, 2, 64, 32, 33, True),  # window one more than the tile width
    (2, 300, 6, 2, 64, 64, 100, True),  # several query blocks, window over several tiles
    (1, 160, 4, 4, 128, 128, 48, True),
    (1, 130, 4, 2, 128, 64, 40, True),
    (1, 200, 6, 1, 64, 32, 200, False),  # the GA form: causal, no sink, ratio 6
    (1, 200, 6, 2, 64, 32, 10000, True),  # W far above S
]
NAMES = ("o", "lse", "dq", "dk", "dv", "dsink")
_ATTN = {}


def attn_case(B, S, Hq, Hkv, D, DV, W, sink):
    """Operands and both flows of the restatement, computed once per case and shared (never modified) by the tests."""
    key = (B, S, Hq, Hkv, D, DV, min(W, S), sink)
    if key not in _ATTN:
        q, k, v, do, z = O.attn_operands(B, S, Hq, Hkv, D, DV, seed=7000 + S + D + Hq + DV, sink=sink)
        c = {"ops": (q, k, v, do, z)}
        for exact in (False, True):
            out, lse = O.sink_attention(q, k, v, W, z, exact)
            dq, dk, dv, dz = O.sink_attention_bwd(q, k, v, do, W, z, exact)
            c[exact] = dict(o=out, lse=lse, dq=dq, dk=dk, dv=dv, dsink=dz)
        _ATTN[key] = c
    return _ATTN[key]


def _run_attn(q, k, v, do, z, W, parts=None):
    """The kernels on [B, H, S, .] operands -> dict of [B, H, S, .] results (lse [B, Hq, S], dsink fp32 [Hq] or None)."""
    KM = _km()
    B, Hq, S, D = q.shape
    Hkv, DV = k.shape[1], v.shape[3]
    qt, kt, vt, dot = [O.to_tokens(t).cuda() for t in (q, k, v, do)]
    zd = None if z is None else z.cuda()
    o, lse = KM.sink_attn_fwd(qt, kt, vt, B, S, Hq, Hkv, D, DV, W, sink=zd)
    dq, dk, dv, dz = KM.sink_attn_bwd(qt, kt, vt, o, dot, lse, B, S, Hq, Hkv, D, DV, W, sink=zd, parts=parts)
    return dict(o=O.from_tokens(o, B, S, Hq, DV), lse=lse, dq=O.from_tokens(dq, B, S, Hq, D), dk=O.from_tokens(dk, B, S, Hkv, D),
                dv=O.from_tokens(dv, B, S, Hkv, DV), dsink=dz)


def _same_bits(a, b, names=NAMES):
    for name in names:
        if a[name] is None or b[name] is None:
            assert a[name] is None and b[name] is None, name
        else:
            assert torch.equal(a[name], b[name]), name


@pytest.mark.parametrize("B,S,Hq,Hkv,D,DV,W,sink", ATTN_CASES)
def test_sink_attention_against_fp64_restatement(B, S, Hq, Hkv, D, DV, W, sink):
    c = attn_case(B, S, Hq, Hkv, D, DV, W, sink)
    mine = _run_attn(*c["ops"], W)
    bad = []
    for name in NAMES:
        if name == "dsink" and not sink:
            assert mine["dsink"] is None
            continue
        judge(name, mine[name], c[False][name], c[True][name], bad)
    assert not bad, "\n".join(bad)


def test_no_sink_and_a_sink_far_below_every_score_give_the_same_bits():
    c = attn_case(1, 200, 6, 1, 64, 32, 200, False)
    q, k, v, do, _ = c["ops"]
    a = _run_attn(q, k, v, do, None, 200)
    b = _run_attn(q, k, v, do, torch.full((6,), -30000.0), 200)
    _same_bits(a, b, NAMES[:5])
    assert a["dsink"] is None and bool((b["dsink"] == 0).all())  # exp(z - lse) underflows to nothing
    for W in (7, 64):
        _same_bits(_run_attn(q, k, v, do, None, W), _run_attn(q, k, v, do, torch.full((6,), -30000.0, dtype=F32), W), NAMES[:5])


def test_every_window_at_or_above_the_sequence_length_is_plain_causal_attention():
    c = attn_case(1, 200, 6, 2, 64, 32, 10000, True)
    a, b = _run_attn(*c["ops"], 200), _run_attn(*c["ops"], 10000)
    _same_bits(a, b)
    _same_bits(a, _run_attn(*c["ops"], 2**40))


def test_a_sink_far_above_every_score_takes_the_softmax():
    q, k, v, do, _ = O.attn_operands(1, 70, 6, 2, 64, 32, seed=31)
    z = torch.full((6,), 30.0)
    r = _run_attn(q, k, v, do, z, 24)
    for name in NAMES:
        assert bool(torch.isfinite(r[name].float()).all()), name
    assert float((r["lse"].cpu() - 30.0).abs().max()) < 1e-3  # log(e^30 + sum e^s) - 30 < 1e-9: what is left is the kernel's own rounding
    assert float(r["o"].float().abs().max()) < 1e-6


def test_a_window_of_one_scales_the_value():
    """W = 1, Hq = Hkv, D = DV: o = v / (1 + exp(z - s)) with s = scale * q . k of the token itself."""
    B, S, H, D = 2, 70, 3, 64
    q, k, v, do, z = O.attn_operands(B, S, H, H, D, D, seed=11)
    r = _run_attn(q, k, v, do, z, 1)
    s = (q.double() * k.double()).sum(-1) * D ** -0.5
    zz = z.double().view(1, H, 1)
    bad = []
    judge("o", r["o"], O.sink_attention(q, k, v, 1, z)[0], v.double() / (1 + torch.exp(zz - s)).unsqueeze(-1), bad)
    judge("lse", r["lse"], O.sink_attention(q, k, v, 1, z)[1], torch.log(torch.exp(s) + torch.exp(zz)), bad)
    assert not bad, "\n".join(bad)


def test_keys_outside_the_window_do_not_reach_the_result():
    """Locality at (1, 300, 6, 2, 64, 32, 50) with a sink: with K and V rows 0..99 replaced by other finite values (some of magnitude 1e4), queries
    >= 149 keep O and lse bit for bit; with dO zeroed for queries < 149, dK and dV of rows 0..99 are exactly zero."""
    B, S, Hq, Hkv, D, DV, W = 1, 300, 6, 2, 64, 32, 50
    q, k, v, do, z = O.attn_operands(B, S, Hq, Hkv, D, DV, seed=12)
    g = torch.Generator().manual_seed(13)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, :100] = torch.randn(B, Hkv, 100, D, generator=g).to(BF16)
    v2[:, :, :100] = torch.randn(B, Hkv, 100, DV, generator=g).to(BF16)
    k2[:, :, 90:100, ::7] = 1e4
    v2[:, :, 80:100, ::5] = -1e4
    v2[:, :, :5, ::3] = 1e4
    do2 = do.clone()
    do2[:, :, :149] = 0
    a, b = _run_attn(q, k, v, do2, z, W), _run_attn(q, k2, v2, do2, z, W)
    assert torch.equal(a["o"][:, :, 149:], b["o"][:, :, 149:]) and torch.equal(a["lse"][:, :, 149:], b["lse"][:, :, 149:])
    assert bool(torch.isfinite(b["o"].float()).all()) and bool(torch.isfinite(b["lse"]).all())
    for r in (a, b):
        assert bool((r["dk"][:, :, :100] == 0).all()) and bool((r["dv"][:, :, :100] == 0).all())
    assert float(b["dk"][:, :, 100:].float().abs().sum()) > 0
    assert torch.equal(a["dsink"], b["dsink"])  # queries < 149 have delta = 0, the others did not see the replaced rows


def test_attention_backward_is_bit_reproducible():
    c = attn_case(2, 300, 6, 2, 64, 64, 100, True)
    a, b = _run_attn(*c["ops"], 100), _run_attn(*c["ops"], 100)
    _same_bits(a, b)
    bad = []
    small = _run_attn(*c["ops"], 100, parts=2)  # two workgroups fold all 600 rows of every head
    judge("dsink (2 workgroups)", small["dsink"], c[False]["dsink"], c[True]["dsink"], bad)
    _same_bits(small, _run_attn(*c["ops"], 100, parts=2))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("W", [1, 33, 130])
@pytest.mark.parametrize("D", [64, 128])
def test_the_windowed_entry_points_are_the_sink_kernels_at_equal_head_dims_without_a_sink(D, W):
    """mi355_swa_attn_* and mi355_sink_attn_* at DV = D without a sink are two ABI names of one kernel (csrc/attention_band.hip): same bits.
    S = 130 is two query blocks, the second of two rows, and five key tiles, the last ragged; W crosses one key, a tile edge and W = S."""
    from llm_quest_amd import kernels_g3 as KG

    KM = _km()
    B, S, Hq, Hkv = 2, 130, 4, 2
    q, k, v, do = [O.to_tokens(t).cuda() for t in O.attn_operands(B, S, Hq, Hkv, D, D, seed=9100 + D, sink=False)[:4]]
    o_s, lse_s = KM.sink_attn_fwd(q, k, v, B, S, Hq, Hkv, D, D, W)
    o_w, lse_w = KG.swa_attn_fwd(q, k, v, B, S, Hq, Hkv, D, W)
    assert torch.equal(o_s, o_w) and torch.equal(lse_s, lse_w)
    dq_s, dk_s, dv_s, dz = KM.sink_attn_bwd(q, k, v, o_s, do, lse_s, B, S, Hq, Hkv, D, D, W)
    dq_w, dk_w, dv_w = KG.swa_attn_bwd(q, k, v, o_w, do, lse_w, B, S, Hq, Hkv, D, W)
    assert dz is None
    assert torch.equal(dq_s, dq_w) and torch.equal(dk_s, dk_w) and torch.equal(dv_s, dv_w)
    assert float(o_s.float().abs().sum()) > 0 and float(dk_s.float().abs().sum()) > 0  # the launches wrote something


@pytest.mark.parametrize("B,S,Hq,Hkv,D,DV,W", [(1, 1, 2, 1, 64, 32, 1), (2, 70, 6, 2, 64, 32, 5), (1, 129, 4, 2, 128, 64, 33), (1, 40, 2, 1, 192, 128, 16)])
def test_attention_outputs_stay_inside_their_buffers(B, S, Hq, Hkv, D, DV, W):
    from llm_quest_amd import _lib as L

    KM = _km()
    dev = torch.device("cuda")
    q, k, v, do, z = O.attn_operands(B, S, Hq, Hkv, D, DV, seed=21)
    q, k, v, do = [O.to_tokens(t).cuda() for t in (q, k, v, do)]
    z = z.float().cuda()
    T, parts = B * S, 3
    shapes = dict(o=((T, Hq * DV), BF16), lse=((B, Hq, S), F32), delta=((B, Hq, S), F32), dq=((T, Hq * D), BF16), dk=((T, Hkv * D), BF16),
                  dv=((T, Hkv * DV), BF16), part=((parts, Hq), F32))
    outs = {n: _padded(s, dt, dev) for n, (s, dt) in shapes.items()}
    w = {n: o[1] for n, o in outs.items()}
    p = L.ptr
    L.require_gpu(q)
    L.call("mi355_sink_attn_fwd", B, S, Hq, Hkv, D, DV, W, p(q), Hq * D, p(k), Hkv * D, p(v), Hkv * DV, p(z), p(w["o"]), Hq * DV, p(w["lse"]), D ** -0.5)
    L.call("mi355_sink_attn_bwd", B, S, Hq, Hkv, D, DV, W, p(q), Hq * D, p(k), Hkv * D, p(v), Hkv * DV, p(w["o"]), Hq * DV, p(do), Hq * DV, p(z), p(w["lse"]),
           p(w["delta"]), p(w["dq"]), Hq * D, p(w["dk"]), Hkv * D, p(w["dv"]), Hkv * DV, p(w["part"]), parts, D ** -0.5)
    _check_padded(outs)
    o, lse = KM.sink_attn_fwd(q, k, v, B, S, Hq, Hkv, D, DV, W, sink=z)  # the same launches through the wrappers give the same bits
    dq, dk, dv, dz = KM.sink_attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, DV, W, sink=z, parts=parts)
    assert torch.equal(o, w["o"]) and torch.equal(lse, w["lse"]) and torch.equal(dq, w["dq"]) and torch.equal(dk, w["dk"]) and torch.equal(dv, w["dv"])
    assert torch.equal(dz, L.reduce_rows(w["part"].contiguous()))


def test_the_released_pair_192_128_meets_the_rule():
    c = attn_case(1, 70, 4, 2, 192, 128, 24, True)
    mine = _run_attn(*c["ops"], 24)
    bad = []
    for name in NAMES:
        judge(name, mine[name], c[False][name], c[True][name], bad)
    assert not bad, "\n".join(bad)


def test_bad_attention_arguments_come_back_as_codes_with_messages():
    from llm_quest_amd import _lib as L

    KM = _km()
    lib = L.load()
    t = torch.zeros(8, 384, dtype=BF16, device="cuda")
    f = torch.zeros(64, dtype=F32, device="cuda")
    q, s = t.data_ptr(), None
    cases = [
        (lambda: lib.mi355_sink_attn_fwd(1, 8, 6, 2, 96, 32, 4, q, 576, q, 192, q, 64, None, q, 192, f.data_ptr(), 0.1, s), b"(96, 32) not built"),
        (lambda: lib.mi355_sink_attn_fwd(1, 8, 6, 2, 64, 32, 0, q, 384, q, 128, q, 64, None, q, 192, f.data_ptr(), 0.1, s), b"window 0"),
        (lambda: lib.mi355_sink_attn_fwd(1, 8, 6, 4, 64, 32, 4, q, 384, q, 256, q, 128, None, q, 192, f.data_ptr(), 0.1, s), b"multiple of kv heads"),
        (lambda: lib.mi355_sink_attn_fwd(1, 8, 6, 2, 64, 32, 4, q, 384, q + 2, 128, q, 64, None, q, 192, f.data_ptr(), 0.1, s), b"16-byte aligned"),
        (lambda: lib.mi355_sink_attn_fwd(1, 8, 6, 2, 64, 32, 4, q, 384, q, 128, q, 64, None, None, 192, f.data_ptr(), 0.1, s), b"null pointer"),
        (lambda: lib.mi355_sink_attn_bwd(1, 8, 6, 2, 64, 32, 4, q, 384, q, 128, q, 64, q, 192, q, 192, f.data_ptr(), f.data_ptr(), f.data_ptr(), q, 384, q, 128, q, 64,
                                         None, 4, 0.1, s), b"dsink_partial must be given"),
    ]
    for call, msg in cases:
        assert call() != 0 and msg in lib.mi355_last_error(), (msg, lib.mi355_last_error())
    with pytest.raises(ValueError, match="window must be at least 1"):
        KM.sink_attn_fwd(t, t[:, :128], t[:, :64], 1, 8, 6, 2, 64, 32, 0)
    with pytest.raises(ValueError, match=r"\(96, 32\) not built"):
        KM.sink_attn_fwd(t, t[:, :128], t[:, :64], 1, 8, 4, 2, 96, 32, 4)
    with pytest.raises(ValueError, match="multiple of kv heads"):
        KM.sink_attn_fwd(t, t[:, :256], t[:, :128], 1, 8, 6, 4, 64, 32, 4)
    with pytest.raises(ValueError, match="v must be bf16"):
        KM.sink_attn_fwd(t, t[:, :128], t[:, :128], 1, 8, 6, 2, 64, 32, 4)  # v as wide as k: DV is 32 here
    with pytest.raises(ValueError, match="sink must be bf16 or fp32"):
        KM.sink_attn_fwd(t, t[:, :128], t[:, :64], 1, 8, 6, 2, 64, 32, 4, sink=f[:5])
    with pytest.raises(ValueError, match="rotated width 21"):
        KM.normrope_fwd(t, 8, 4, 2, 64, torch.zeros(8, 21, device="cuda"), torch.zeros(8, 21, device="cuda"), t[0, :64].contiguous(), t[0, :64].contiguous())
    with pytest.raises(ValueError, match="head_dim 32 not built"):
        KM.normrope_fwd(t, 8, 4, 2, 32, torch.zeros(8, 20, device="cuda"), torch.zeros(8, 20, device="cuda"), t[0, :32].contiguous(), t[0, :32].contiguous())


# ----------------------------------------------------------------------------------------------------------------- norm + partial RoPE
FACTOR = {(64, 20): 0.33, (64, 64): 1.0, (128, 20): 0.16, (128, 42): 0.33, (128, 128): 1.0}  # RoPE.partial_rotation(D, f), floored to even, = R
SMALL_GRID = 3


@pytest.mark.parametrize("S", [1, 70])
@pytest.mark.parametrize("Hq,Hkv", [(6, 2), (6, 1)])
@pytest.mark.parametrize("D,R", list(FACTOR))
def test_norm_and_partial_rope_against_fp64_restatement(D, R, Hq, Hkv, S):
    """The q and k heads sit in the first (Hq + Hkv) * D columns of a fused [T, (Hq + Hkv) * D + Hkv * DV] projection, as the model passes them."""
    KM = _km()
    B, DV = 2, D // 2
    xq, dyq, wq = O.norm_rope_operands(B, S, Hq, D, seed=500 + S + D + R + Hq)
    xk, dyk, wk = O.norm_rope_operands(B, S, Hkv, D, seed=900 + S + D + R + Hkv)
    cos, sin = O.rope_tables(10000, D, 96, FACTOR[(D, R)])
    assert cos.shape == (96, R)
    ref, ex = {}, {}
    for flow, exact in ((ref, False), (ex, True)):
        flow["yq"], flow["yk"] = O.norm_rope(xq, wq, cos, sin, exact), O.norm_rope(xk, wk, cos, sin, exact)
        flow["dxq"], flow["dwq"] = O.norm_rope_bwd(xq, wq, cos, sin, dyq, exact)
        flow["dxk"], flow["dwk"] = O.norm_rope_bwd(xk, wk, cos, sin, dyk, exact)
    T, nq, nk = B * S, Hq * D, Hkv * D
    qkv = torch.full((T, nq + nk + Hkv * DV), 3.0, dtype=BF16)
    qkv[:, :nq], qkv[:, nq : nq + nk] = O.to_tokens(xq), O.to_tokens(xk)
    dy = torch.cat((O.to_tokens(dyq), O.to_tokens(dyk)), dim=1).cuda()
    qkv_d, cos_d, sin_d, wq_d, wk_d = qkv.cuda(), cos.cuda(), sin.cuda(), wq.cuda(), wk.cuda()
    y = KM.normrope_fwd(qkv_d, S, Hq, Hkv, D, cos_d, sin_d, wq_d, wk_d)
    assert y.shape == (T, nq + nk)
    bad = []
    judge("yq", O.from_tokens(y[:, :nq], B, S, Hq, D), ref["yq"], ex["yq"], bad)
    judge("yk", O.from_tokens(y[:, nq:], B, S, Hkv, D), ref["yk"], ex["yk"], bad)
    # features >= R are the normalised input: the same bits as a run whose tables rotate by nothing (cos = 1, sin = 0)
    plain = KM.normrope_fwd(qkv_d, S, Hq, Hkv, D, torch.ones_like(cos_d), torch.zeros_like(sin_d), wq_d, wk_d)
    tail = lambda t: t.view(T, Hq + Hkv, D)[:, :, R:]
    assert torch.equal(tail(y), tail(plain))
    judge("norm alone, q", O.from_tokens(plain[:, :nq], B, S, Hq, D), O.rms_norm(xq, wq), O.rms_norm(xq, wq, True), bad)
    dqkv = torch.full_like(qkv_d, 5.0)
    dx, dwq, dwk = KM.normrope_bwd(qkv_d, dy, S, Hq, Hkv, D, cos_d, sin_d, wq_d, wk_d, dx=dqkv)
    assert dx.data_ptr() == dqkv.data_ptr() and bool((dqkv[:, nq + nk :] == 5.0).all())  # the v columns belong to the attention backward
    assert bool((qkv_d[:, nq + nk :] == 3.0).all())
    judge("dxq", O.from_tokens(dqkv[:, :nq], B, S, Hq, D), ref["dxq"], ex["dxq"], bad)
    judge("dxk", O.from_tokens(dqkv[:, nq : nq + nk], B, S, Hkv, D), ref["dxk"], ex["dxk"], bad)
    judge("dwq", dwq, ref["dwq"], ex["dwq"], bad)
    judge("dwk", dwk, ref["dwk"], ex["dwk"], bad)
    if S == 70:  # a small grid of partial rows, and the same bits twice
        _, g3q, g3k = KM.normrope_bwd(qkv_d, dy, S, Hq, Hkv, D, cos_d, sin_d, wq_d, wk_d, parts=SMALL_GRID)
        _, g4q, g4k = KM.normrope_bwd(qkv_d, dy, S, Hq, Hkv, D, cos_d, sin_d, wq_d, wk_d, parts=SMALL_GRID)
        judge(f"dwq ({SMALL_GRID} workgroups)", g3q, ref["dwq"], ex["dwq"], bad)
        judge(f"dwk ({SMALL_GRID} workgroups)", g3k, ref["dwk"], ex["dwk"], bad)
        assert torch.equal(g3q, g4q) and torch.equal(g3k, g4k)
    assert not bad, "\n".join(bad)


def test_norm_rope_outputs_stay_inside_their_buffers():
    from llm_quest_amd import _lib as L

    B, S, Hq, Hkv, D, R, parts = 2, 7, 3, 1, 64, 20, 2
    dev = torch.device("cuda")
    x, dy, w = O.norm_rope_operands(B, S, Hq + Hkv, D, seed=77)
    xt, dyt, wd = O.to_tokens(x).cuda(), O.to_tokens(dy).cuda(), w.cuda()
    cos, sin = [t.cuda() for t in O.rope_tables(10000, D, 16, 0.33)]
    T, width = B * S, (Hq + Hkv) * D
    outs = {n: _padded(s, dt, dev) for n, (s, dt) in dict(y=((T, width), BF16), dx=((T, width), BF16), part=((parts, 2 * D), F32)).items()}
    v = {n: o[1] for n, o in outs.items()}
    p = L.ptr
    L.require_gpu(xt)
    L.call("mi355_mimo_normrope_fwd", T, S, Hq, Hkv, D, R, p(xt), width, p(wd), p(wd), p(cos), p(sin), 16, p(v["y"]), width, 1e-6)
    L.call("mi355_mimo_normrope_bwd", T, S, Hq, Hkv, D, R, p(xt), width, p(wd), p(wd), p(cos), p(sin), 16, p(dyt), width, p(v["dx"]), width, p(v["part"]), parts, 1e-6)
    _check_padded(outs)


# ----------------------------------------------------------------------------------------------------------------- model on the fixture
@pytest.fixture(scope="module")
def fixture():
    return O.load_fixture()


def _model(t):
    from llm_quest_amd.xiaomi.mimo_v2_flash_model import MiMoModel

    torch.manual_seed(0)
    m = MiMoModel(dict(CFG)).to(BF16)
    res = m.load_state_dict({k[3:]: v for k, v in t.items() if k.startswith("sd.")}, strict=False)
    assert not res.unexpected_keys and all(k.split(".")[-1].split("_")[0] in ("mask", "cos", "sin") for k in res.missing_keys)
    return m.cuda().train()


def _force(m, t):
    for i in LAYERS:
        m.main_model.layers[i].feed_forward._forced_topk = t[f"moe.{i}.topk_idxs"].cuda()


def test_model_on_the_fixture_with_the_selection_forced(fixture):
    import deepseek_moe_oracle as MO

    t = fixture
    m = _model(t)
    _force(m, t)
    ids, tgt = t["in.ids"].cuda(), t["in.targets"].cuda()
    loss = m(ids, tgt)
    assert loss.dtype == BF16 and loss.dim() == 0  # the logits' dtype, as F.cross_entropy on bf16 logits
    loss.backward()
    bad = []
    for i in LAYERS:
        ffn, pre = m.main_model.layers[i].feed_forward, f"moe.{i}."
        assert torch.equal(ffn._routed[0].cpu(), t[pre + "topk_idxs"]) and torch.equal(ffn._routed[1].cpu(), t[pre + "counts"]), i
        assert torch.equal(ffn.biases.cpu(), t[pre + "biases"]), f"layer {i}: updated biases"
        judge(pre + "max_vio", ffn.max_vio.reshape(1), t[pre + "max_vio"], MO.max_violation(t[pre + "counts"].long(), torch.float64).reshape(1), bad)
    judge("loss", loss.reshape(1), t["out.loss"].reshape(1), t["twin.loss"].reshape(1), bad)
    with open(os.path.join(O.GOLDEN, "mimo_signatures.json")) as f:
        floors = json.load(f)["floors"]
    judged = 0
    for name, p in m.named_parameters():
        if name.startswith("mtp_modules.") and ".out_layer." in name:
            continue
        assert p.grad is not None, name
        if "grad." + name not in t:  # an expert that received no token: the reference leaves None, here an exactly zero gradient
            assert ".routed_experts." in name and bool((p.grad == 0).all()), name
            continue
        floor = O.rel_l2(t["grad." + name], t["twin.grad." + name])
        assert abs(floor - floors[name]) <= 1e-3 * max(floor, 1e-30) + 1e-12, name
        if floor <= 0.1:
            judge("d " + name, p.grad, t["grad." + name], t["twin.grad." + name], bad)
            judged += 1
    want = sum(1 for v in floors.values() if v <= 0.1)
    print(f"  {judged} gradients judged of {len(floors)}")
    assert judged == want and judged >= 0.9 * len(floors)
    owners = [(blk, blk._arena) for blk in m.main_model.layers] + [(mod, mod._own_arena) for mod in m.mtp_modules]
    for mod, arena in owners:  # every block's gradients lie inside its arena
        lo, hi = arena.grad.data_ptr(), arena.grad.data_ptr() + arena.grad.numel() * 2
        for name, p in mod.named_parameters():
            if not name.startswith("out_layer."):
                assert lo <= p.grad.data_ptr() < hi, name
    m.eval()
    with torch.no_grad():
        logits = m(ids)
        main_loss = m(ids, tgt)
    judge("logits", logits, t["out.logits"], t["twin.logits"], bad)
    # eval with targets: the main loss only
    # eval with targets: the main loss only -- the cross entropy of these very logits, rounded once to bf16 (half an ulp: 2^-9 relative)
    ce = float(torch.nn.functional.cross_entropy(logits.double().flatten(0, 1).cpu(), t["in.targets"].flatten()))
    assert main_loss.dtype == BF16 and abs(float(main_loss) - ce) <= 2.0 ** -8 * ce and float(main_loss) < float(loss.detach())
    assert not bad, "\n".join(bad)


def test_an_expert_without_a_token_ends_with_exactly_zero_gradients(fixture):
    t = fixture
    m = _model(t)
    _force(m, t)
    layer, E = LAYERS[0], CFG["num_experts"]
    idx = t[f"moe.{layer}.topk_idxs"].clone().long()
    victim = 5
    other = (idx.sum(dim=1, keepdim=True) + 1) % E  # an expert per token ...
    for _ in range(3):  # ... that is neither the victim nor already selected
        clash = (other == victim) | (other == idx).any(dim=1, keepdim=True)
        other = torch.where(clash, (other + 1) % E, other)
    assert not bool(((other == victim) | (other == idx).any(dim=1, keepdim=True)).any())
    idx = torch.where(idx == victim, other.expand_as(idx), idx)
    m.main_model.layers[layer].feed_forward._forced_topk = idx.int().cuda()
    m(t["in.ids"].cuda(), t["in.targets"].cuda()).backward()
    ffn = m.main_model.layers[layer].feed_forward
    assert int(ffn._routed[1][victim]) == 0
    for e, ex in enumerate(ffn.routed_experts):
        for name, p in ex.named_parameters():
            assert bool(torch.isfinite(p.grad).all()) and bool((p.grad == 0).all()) == (e == victim), (e, name)


def test_model_on_the_fixture_with_normal_routing(fixture):
    """Only the first MoE layer is judged against the fixture's selection: a deeper layer's input already carries the rounding differences of the
    layers before it, so its logits are no longer the reference's to within one ulp."""
    t = fixture
    m = _model(t)
    loss = m(t["in.ids"].cuda(), t["in.targets"].cuda())
    loss.backward()
    assert bool(torch.isfinite(loss))
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    first = m.main_model.layers[LAYERS[0]].feed_forward
    assert float(first.gate.weight.grad.float().abs().max()) > 0 and float(first.gate.bias.grad.float().abs().max()) > 0
    for blk in m.main_model.layers:
        if blk.use_sliding_window:
            assert float(blk.att.sink.grad.float().abs().max()) > 0
    pre = f"moe.{LAYERS[0]}."
    robust = t[pre + "robust"].bool()
    mine, ref = first._routed[0].cpu().long().sort(dim=1).values, t[pre + "topk_idxs"].long().sort(dim=1).values
    same = (mine == ref).all(dim=1)
    print(f"  first MoE layer: {int(robust.sum())} of {robust.numel()} tokens robust; the selection agrees on {int(same.sum())}")
    assert int(robust.sum()) * 10 >= 9 * robust.numel() and bool(same[robust].all())
    for i in LAYERS:
        assert bool(torch.isfinite(m.main_model.layers[i].feed_forward.max_vio))


@pytest.mark.parametrize("layer", [1, 2])
def test_kernels_on_the_captured_attention_operands(fixture, layer):
    """The reference's own q, k (after norm + RoPE), v of a sliding-window layer (1: window 24, the sink, ratio 3) and a global one (2: causal, no
    sink, ratio 6) through the kernels, against the reference's context and the fp64 restatement."""
    t = fixture
    q, k, v, ctx = [t[f"cap.{layer}.{n}"] for n in ("q", "k", "v", "ctx")]
    swa = O.is_swa(CFG, layer)
    assert swa == (layer == 1) and k.shape[1] == (CFG["num_swa_kv_groups"] if swa else CFG["num_ga_kv_groups"])
    z = t[f"sd.main_model.layers.{layer}.att.sink"] if swa else None
    W = CFG["window_size"] if swa else q.shape[2]
    mine = _run_attn(q, k, v, torch.zeros_like(ctx), z, W)
    bad = []
    judge(f"layer {layer} context", mine["o"], ctx, O.sink_attention(q, k, v, W, z, True)[0], bad)
    assert not bad, "\n".join(bad)


def test_twenty_optimizer_steps_lower_the_loss(fixture):
    from llm_quest_amd.optim import ArenaAdamW

    t = fixture
    m = _model(t)
    ids, tgt = t["in.ids"].cuda(), t["in.targets"].cuda()
    opt = ArenaAdamW(m.parameters(), lr=1e-3, weight_decay=0.0).attach(m)
    sinks = [blk.att.sink.detach().clone() for blk in m.main_model.layers if blk.use_sliding_window]
    losses = []
    for step in range(21):
        loss = m(ids, tgt)
        losses.append(loss.detach())
        if step == 20:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    first, last = float(losses[0]), float(losses[-1])
    print(f"  loss at step 0: {first:.4f}, at step 20: {last:.4f}")
    assert last == last and last < first
    now = [blk.att.sink.detach() for blk in m.main_model.layers if blk.use_sliding_window]
    assert all(not torch.equal(a, b) for a, b in zip(sinks, now))  # the sinks train


@pytest.mark.parametrize("window", [24, None])
def test_attention_module_on_its_own(window):
    """GroupedQueryAttentionWithSink outside a block: the window comes from the mask it is handed (a band of 24 with the sink, the causal mask
    without one); output, dx and every parameter gradient against the restatement's autograd."""
    from llm_quest_amd.common.buffers import GlobalBuffers
    from llm_quest_amd.xiaomi.mimo_v2_flash_attention import GroupedQueryAttentionWithSink

    swa = window is not None
    B, S, d = 2, 70, 128
    Hq, Hkv, D, DV = 6, 2 if swa else 1, 64, 32
    torch.manual_seed(5)
    att = GroupedQueryAttentionWithSink(d, Hq, Hkv, D, value_head_dim=DV, dtype=BF16, is_sliding_window=swa)
    g = torch.Generator().manual_seed(6)
    O.perturb_parameters(list(att.named_parameters()), g)
    x = torch.randn(B, S, d, generator=g).to(BF16)
    dy = torch.randn(B, S, d, generator=g).to(BF16)
    cfg = dict(n_heads=Hq, num_swa_kv_groups=Hkv, num_ga_kv_groups=Hkv, head_dim=D, value_head_dim=DV, window_size=window)
    cos, sin = O.rope_tables(10000, D, 96, 0.33)
    sd = {k: v.detach().clone() for k, v in att.state_dict().items()}
    flows = {}
    for exact in (False, True):
        leaves = {k: O._c(v, exact).detach().clone().requires_grad_(True) for k, v in sd.items()}
        xg = O._c(x, exact).detach().clone().requires_grad_(True)
        y = O.attention(leaves, "", xg, cfg, swa, cos, sin, exact)
        grads = torch.autograd.grad(y, [xg] + list(leaves.values()), O._c(dy, exact))
        flows[exact] = dict(y=y.detach(), dx=grads[0], **{"d " + k: g_ for k, g_ in zip(leaves, grads[1:])})
    mask = (GlobalBuffers.get_swa_mask(96, window) if swa else GlobalBuffers.get_causal_mask(96)).cuda()
    att = att.cuda()
    xd = x.cuda().requires_grad_(True)
    y = att(xd, mask, cos.cuda(), sin.cuda())
    y.backward(dy.cuda())
    bad = []
    judge("y", y, flows[False]["y"], flows[True]["y"], bad)
    judge("dx", xd.grad, flows[False]["dx"], flows[True]["dx"], bad)
    for name, p in att.named_parameters():
        judge("d " + name, p.grad, flows[False]["d " + name], flows[True]["d " + name], bad)
    assert swa == hasattr(att, "sink")
    with torch.no_grad():
        assert torch.equal(att(xd, mask, cos.cuda(), sin.cuda()), y)  # the no-grad forward: the same bits
    assert not bad, "\n".join(bad)
