"""DeepSeek-V3 kernels (csrc/deepseek.hip), MultiLatentAttention and the dense DeepSeekV3Model on the GPU, against the plain-torch
restatement (tests/deepseek_oracle.py) and the reference fixtures (tests/golden/deepseek_tiny*, deepseek_mla*).

Tolerance: the project's 1.5x rule and nothing else -- the relative L2 distance of a kernel output to the fp64
restatement is at most 1.5 x the distance of the reference-dtype-flow restatement to the same fp64 result, with 2e-3 absolute slack only
where that floor is below 1e-2.  Where the fp64 result is identically zero (every gradient of q and k at S = 1: a one-key softmax) a
relative distance does not exist; the kernel is then held to 1e-6 absolute per element.
"""

import pytest
import torch

import deepseek_oracle as DO

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
PAIRS = [(64, 32), (128, 64)]
SHAPES = [(1, 1, 1), (2, 31, 2), (1, 33, 3), (2, 70, 2), (1, 129, 2), (1, 200, 12)]  # (B, S, Hq)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _km():
    from llm_quest_amd import kernels_mla as KM

    return KM


def judge(name, mine, ref_flow, exact, report):
    mine, ref_flow, exact = mine.detach().cpu(), ref_flow.detach().cpu(), exact.detach().cpu()
    assert mine.shape == exact.shape, (name, mine.shape, exact.shape)
    if float(exact.double().norm()) == 0.0:
        worst = float(mine.double().abs().max())
        print(f"  {name}: exact value is zero; kernel max |x| {worst:.3e}")
        if not worst <= 1e-6:
            report.append(f"{name}: exact value is zero, kernel max |x| {worst:.3e} > 1e-6")
        return
    floor = DO.rel_l2(ref_flow, exact)
    got = DO.rel_l2(mine, exact)
    bound = 1.5 * floor + (0.0 if floor >= 1e-2 else 2e-3)
    print(f"  {name}: kernel {got:.3e}  reference flow {floor:.3e}  bound {bound:.3e}")
    if not got <= bound:
        report.append(f"{name}: {got:.3e} > {bound:.3e} (floor {floor:.3e})")


# ----------------------------------------------------------------------------------------------------------------- attention
NAMES = ("o", "lse", "dq_nope", "dq_rope", "dk_nope", "dk_rope", "dv")
_CASES = {}


def attn_case(B, S, H, Dn, Dr):
    """Operands and both flows of the restatement, computed once per case and shared (never modified) by the tests."""
    key = (B, S, H, Dn, Dr)
    if key not in _CASES:
        ops = DO.mla_operands(B, S, H, Dn, Dr, seed=9000 + S + Dn + H)
        c = {"ops": ops}
        for dtype in (None, torch.float64):
            o, lse = DO.mla_attention(*ops[:5], dtype=dtype)
            grads = DO.mla_attention_bwd(*ops, dtype=dtype)
            c[dtype] = dict(zip(NAMES, (o, lse) + tuple(grads)))
        _CASES[key] = c
    return _CASES[key]


def _identity_tables(S, Dr):
    return torch.ones(S, Dr, dtype=F32, device="cuda"), torch.zeros(S, Dr, dtype=F32, device="cuda")


def _slices(widths, T, pad, dev, fill=None):
    """Column slices of ONE wider bf16 buffer [T, sum(widths) + pads], 16-byte aligned starts, ``pad`` unused columns between them."""
    total = sum(w + pad for w in widths) + pad
    buf = torch.empty(T, total, dtype=BF16, device=dev) if fill is None else torch.full((T, total), fill, dtype=BF16, device=dev)
    out, c = [], pad
    for w in widths:
        out.append(buf[:, c : c + w])
        c += w + pad
    return buf, out


def run_mla(ops, sliced=False):
    """The kernels on [B, H, S, D] operands (shared key [B, S, Dr]) -> dict of results in the oracle's layouts; dk_rope after the head sum, taken
    through ``mla_rope_bwd`` with identity tables (cos = 1, sin = 0).  ``sliced``: every operand and every bf16 result is a column slice of a
    wider buffer (leading dimension > its row)."""
    KM = _km()
    q_nope, q_rope, k_nope, k_rope, v, do = ops
    B, H, S, Dn = q_nope.shape
    Dr = q_rope.shape[-1]
    T = B * S
    tok = [DO.to_tokens(t) for t in (q_nope, q_rope, k_nope)] + [k_rope.reshape(T, Dr)] + [DO.to_tokens(t) for t in (v, do)]
    dests = {}
    if sliced:
        _, dev_ops = _slices([t.shape[1] for t in tok], T, 24, "cuda")
        for d, s in zip(dev_ops, tok):
            d.copy_(s)
        _, outs = _slices([H * Dn, H * Dn, H * Dr, H * Dn, H * Dn], T, 8, "cuda")
        dests = dict(o=outs[0], dq_nope=outs[1], dq_rope=outs[2], dk_nope=outs[3], dv=outs[4])
    else:
        dev_ops = [t.cuda() for t in tok]
    qn, qr, kn, kr, vv, dd = dev_ops
    o, lse = KM.mla_attn_fwd(qn, qr, kn, kr, vv, B, S, H, Dn, Dr, o=dests.get("o"))
    dqn, dqr, dkn, dkh, dv = KM.mla_attn_bwd(qn, qr, kn, kr, vv, o, dd, lse, B, S, H, Dn, Dr, dq_nope=dests.get("dq_nope"), dq_rope=dests.get("dq_rope"),
                                             dk_nope=dests.get("dk_nope"), dv=dests.get("dv"))
    cos, sin = _identity_tables(S, Dr)
    _, dkr = KM.mla_rope_bwd(dqr, dkh, S, H, Dr, cos, sin)
    ft = DO.from_tokens
    return dict(o=ft(o, B, S, H, Dn), lse=lse, dq_nope=ft(dqn, B, S, H, Dn), dq_rope=ft(dqr, B, S, H, Dr), dk_nope=ft(dkn, B, S, H, Dn),
                dk_rope=dkr.view(B, S, Dr), dv=ft(dv, B, S, H, Dn), dk_heads=dkh)


@pytest.mark.parametrize("sliced", [False, True], ids=["packed", "sliced"])
@pytest.mark.parametrize("Dn,Dr", PAIRS)
@pytest.mark.parametrize("B,S,H", SHAPES)
def test_attention_against_fp64_restatement(B, S, H, Dn, Dr, sliced):
    c = attn_case(B, S, H, Dn, Dr)
    mine = run_mla(c["ops"], sliced)
    bad = []
    for name in NAMES:
        judge(name, mine[name], c[None][name], c[torch.float64][name], bad)
    assert not bad, "\n".join(bad)
    if sliced:  # the same numbers in the same order: the leading dimension changes addresses only
        packed = run_mla(c["ops"], False)
        for name in NAMES:
            assert torch.equal(mine[name], packed[name]), name


@pytest.mark.parametrize("Dn,Dr", PAIRS)
def test_the_shared_key_is_shared(Dn, Dr):
    """Hq = 3 equals three Hq = 1 runs on each head's slices with the same k_rope: bit for bit in the forward and in the per-head gradients,
    and the summed dk_rope is the fixed-order sum (head 0 + head 1 + head 2, fp32, one rounding) of the three single-head dk_rope's."""
    B, S, H = 1, 33, 3
    ops = attn_case(B, S, H, Dn, Dr)["ops"]
    full = run_mla(ops)
    acc = torch.zeros(B * S, Dr, dtype=F32, device="cuda")
    for h in range(H):
        one = run_mla(tuple(t if i == 3 else t[:, h : h + 1].contiguous() for i, t in enumerate(ops)))
        for name in ("o", "lse", "dq_nope", "dq_rope", "dk_nope", "dv"):
            assert torch.equal(one[name][:, 0], full[name][:, h]), (name, h)
        assert torch.equal(one["dk_heads"][:, 0], full["dk_heads"][:, h]), h
        acc = acc + one["dk_heads"][:, 0]
    assert torch.equal(full["dk_rope"].reshape(B * S, Dr), acc.to(BF16))


@pytest.mark.parametrize("Dn,Dr", PAIRS)
def test_causality(Dn, Dr):
    """Changing keys and values after position i leaves rows <= i of o and lse bit-identical."""
    B, S, H, i = 2, 70, 2, 40
    q_nope, q_rope, k_nope, k_rope, v, do = attn_case(B, S, H, Dn, Dr)["ops"]
    g = torch.Generator().manual_seed(5)
    k2, kr2, v2 = k_nope.clone(), k_rope.clone(), v.clone()
    k2[:, :, i + 1 :] = torch.randn(B, H, S - i - 1, Dn, generator=g).to(BF16) * 3
    kr2[:, i + 1 :] = torch.randn(B, S - i - 1, Dr, generator=g).to(BF16) * 3
    v2[:, :, i + 1 :] = 1e4
    a, b = run_mla((q_nope, q_rope, k_nope, k_rope, v, do)), run_mla((q_nope, q_rope, k2, kr2, v2, do))
    assert torch.equal(a["o"][:, :, : i + 1], b["o"][:, :, : i + 1]) and torch.equal(a["lse"][:, :, : i + 1], b["lse"][:, :, : i + 1])
    assert not torch.equal(a["o"][:, :, i + 1 :], b["o"][:, :, i + 1 :])


@pytest.mark.parametrize("Dn,Dr", PAIRS)
def test_backward_is_reproducible(Dn, Dr):
    ops = attn_case(1, 200, 12, Dn, Dr)["ops"]
    a, b = run_mla(ops), run_mla(ops)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ----------------------------------------------------------------------------------------------------------------- RoPE
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("Dr", [32, 64])
def test_rope_kernels_against_fp64(Dr, H):
    """B = 2, S = 70: the second sample's tokens 70..139 take positions 0..69; inputs are column slices of wider buffers."""
    KM = _km()
    B, S = 2, 70
    T = B * S
    g = torch.Generator().manual_seed(100 + Dr + H)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF16)
    q, k, dq, dkh = rn(B, H, S, Dr), rn(B, S, Dr), rn(B, H, S, Dr), torch.randn(B, H, S, Dr, generator=g)
    cos, sin = DO.rope_tables(10000, Dr, 96)
    _, (qs, ks, dqs) = _slices([H * Dr, Dr, H * Dr], T, 8, "cuda")
    qs.copy_(DO.to_tokens(q)), ks.copy_(k.reshape(T, Dr)), dqs.copy_(DO.to_tokens(dq))
    yq, yk = KM.mla_rope_fwd(qs, ks, S, H, Dr, cos.cuda(), sin.cuda())
    heads = DO.to_tokens(dkh).view(T, H, Dr).contiguous().cuda()
    _, (gq_dst, gk_dst) = _slices([H * Dr, Dr], T, 8, "cuda")
    gq, gk = KM.mla_rope_bwd(dqs, heads, S, H, Dr, cos.cuda(), sin.cuda(), dq_rope_pre=gq_dst, dk_rope_pre=gk_dst)
    bad = []
    ref, ex = DO.mla_rope(q, k, cos, sin), DO.mla_rope(q, k, cos, sin, torch.float64)
    judge("q_rope", DO.from_tokens(yq, B, S, H, Dr), ref[0], ex[0], bad)
    judge("k_rope", yk.view(B, S, Dr), ref[1], ex[1], bad)
    # the head sum is fp32 in the kernel and on fp32 inputs here: the reference flow of the backward is the bf16 rotation of the bf16-rounded sum
    rb = DO.mla_rope_bwd(dq, dkh.sum(dim=1, keepdim=True).to(BF16), cos, sin)
    eb = DO.mla_rope_bwd(dq, dkh, cos, sin, torch.float64)
    judge("dq_rope_pre", DO.from_tokens(gq, B, S, H, Dr), rb[0], eb[0], bad)
    judge("dk_rope_pre", gk.view(B, S, Dr), rb[1], eb[1], bad)
    assert not bad, "\n".join(bad)
    # position = token index inside its sequence: both samples of equal inputs rotate alike
    same = rn(1, H, S, Dr).expand(2, -1, -1, -1)
    yq2, _ = KM.mla_rope_fwd(DO.to_tokens(same).cuda(), ks, S, H, Dr, cos.cuda(), sin.cuda())
    assert torch.equal(yq2[:S], yq2[S:])


# ----------------------------------------------------------------------------------------------------------------- memory safety
def _padded(shape, dtype, dev, pad=64):
    numel = 1
    for s in shape:
        numel *= s
    sentinel = -1024.0  # exact in bf16 and fp32: the same comparison holds for buffers of either type
    buf = torch.full((numel + 2 * pad,), sentinel, dtype=dtype, device=dev)
    return buf, buf[pad : pad + numel].view(shape), sentinel


def _check_padded(outs):
    torch.cuda.synchronize()
    for k, (buf, view, sentinel) in outs.items():
        assert bool((buf[:64] == sentinel).all()) and bool((buf[-64:] == sentinel).all()), f"{k}: written outside its buffer"
        assert not bool((view.float() == sentinel).any()), f"{k}: part of the output was never written"


@pytest.mark.parametrize("Dn,Dr", PAIRS)
@pytest.mark.parametrize("B,S,H", [(1, 1, 1), (2, 31, 2), (1, 33, 3), (1, 129, 2)])
def test_outputs_stay_inside_their_buffers(B, S, H, Dn, Dr):
    from llm_quest_amd import _lib as L

    dev = torch.device("cuda")
    ops = DO.mla_operands(B, S, H, Dn, Dr, seed=31)
    T = B * S
    qn, qr, kn, v, do = [DO.to_tokens(t).cuda() for t in (ops[0], ops[1], ops[2], ops[4], ops[5])]
    kr = ops[3].reshape(T, Dr).cuda()
    wn, wr = H * Dn, H * Dr
    spec = dict(o=((T, wn), BF16), lse=((B, H, S), F32), delta=((B, H, S), F32), dq_nope=((T, wn), BF16), dq_rope=((T, wr), BF16), dk_nope=((T, wn), BF16),
                dk_heads=((T, H, Dr), F32), dv=((T, wn), BF16), q_rope=((T, wr), BF16), k_rope=((T, Dr), BF16), dq_pre=((T, wr), BF16), dk_pre=((T, Dr), BF16))
    outs = {n: _padded(s, dt, dev) for n, (s, dt) in spec.items()}
    w = {n: o[1] for n, o in outs.items()}
    p = L.ptr
    cos, sin = [t.cuda() for t in DO.rope_tables(10000, Dr, max(S, 8))]
    scale = (Dn + Dr) ** -0.5
    L.require_gpu(qn)
    L.call("mi355_mla_rope_fwd", T, S, H, Dr, p(qr), wr, p(kr), Dr, p(cos), p(sin), cos.shape[0], p(w["q_rope"]), wr, p(w["k_rope"]), Dr)
    L.call("mi355_mla_attn_fwd", B, S, H, Dn, Dr, p(qn), wn, p(qr), wr, p(kn), wn, p(kr), Dr, p(v), wn, p(w["o"]), wn, p(w["lse"]), scale)
    L.call("mi355_mla_attn_bwd", B, S, H, Dn, Dr, p(qn), wn, p(qr), wr, p(kn), wn, p(kr), Dr, p(v), wn, p(w["o"]), wn, p(do), wn, p(w["lse"]), p(w["delta"]),
           p(w["dq_nope"]), wn, p(w["dq_rope"]), wr, p(w["dk_nope"]), wn, p(w["dk_heads"]), p(w["dv"]), wn, scale)
    L.call("mi355_mla_rope_bwd", T, S, H, Dr, p(w["dq_rope"]), wr, p(w["dk_heads"]), p(cos), p(sin), cos.shape[0], p(w["dq_pre"]), wr, p(w["dk_pre"]), Dr)
    _check_padded(outs)


def test_operands_past_2_31_bytes_into_an_allocation():
    """The smallest shape whose token offsets pass 2^31 bytes: B = 2, S = 70 (140 tokens) as column slices of a buffer whose rows are 16 MiB
    apart, so every token from 128 on starts more than 2^31 bytes behind its operand's base pointer -- inputs in one such buffer, results in a
    second.  The results equal the packed run's bit for bit."""
    KM = _km()
    B, S, H, Dn, Dr = 2, 70, 2, 64, 32
    T, LD = B * S, (1 << 23) + 8
    need = 2 * T * LD * 2 + (1 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need} bytes of device memory, torch.cuda.mem_get_info() reports {free} free")
    assert (T - 1) * LD * 2 > 1 << 31
    c = attn_case(B, S, H, Dn, Dr)
    q_nope, q_rope, k_nope, k_rope, v, do = c["ops"]
    tok = [DO.to_tokens(t) for t in (q_nope, q_rope, k_nope)] + [k_rope.reshape(T, Dr)] + [DO.to_tokens(t) for t in (v, do)]
    store_in = torch.empty(T * LD, dtype=BF16, device="cuda").view(T, LD)
    store_out = torch.empty(T * LD, dtype=BF16, device="cuda").view(T, LD)
    col, views = 64, []
    for t in tok:
        views.append(store_in[:, col : col + t.shape[1]])
        views[-1].copy_(t)
        col += t.shape[1] + 64
    qn, qr_pre, kn, kr_pre, vv, dd = views
    wn, wr = H * Dn, H * Dr
    o_d, dqn_d, dqr_d, dkn_d, dv_d, qr_d, kr_d, gq_d, gk_d = [store_out[:, a : a + w] for a, w in
                                                             ((64, wn), (256, wn), (448, wr), (576, wn), (768, wn), (960, wr), (1088, Dr), (1152, wr), (1280, Dr))]
    cos, sin = [t.cuda() for t in DO.rope_tables(10000, Dr, 96)]

    def run(qn, qr_pre, kn, kr_pre, vv, dd, dst):
        qr, kr = KM.mla_rope_fwd(qr_pre, kr_pre, S, H, Dr, cos, sin, q_rope=dst.get("qr"), k_rope=dst.get("kr"))
        o, lse = KM.mla_attn_fwd(qn, qr, kn, kr, vv, B, S, H, Dn, Dr, o=dst.get("o"))
        dqn, dqr, dkn, dkh, dv = KM.mla_attn_bwd(qn, qr, kn, kr, vv, o, dd, lse, B, S, H, Dn, Dr, dq_nope=dst.get("dqn"), dq_rope=dst.get("dqr"),
                                                 dk_nope=dst.get("dkn"), dv=dst.get("dv"))
        gq, gk = KM.mla_rope_bwd(dqr, dkh, S, H, Dr, cos, sin, dq_rope_pre=dst.get("gq"), dk_rope_pre=dst.get("gk"))
        return dict(qr=qr, kr=kr, o=o, lse=lse, dqn=dqn, dqr=dqr, dkn=dkn, dkh=dkh, dv=dv, gq=gq, gk=gk)

    far = run(qn, qr_pre, kn, kr_pre, vv, dd, dict(o=o_d, dqn=dqn_d, dqr=dqr_d, dkn=dkn_d, dv=dv_d, qr=qr_d, kr=kr_d, gq=gq_d, gk=gk_d))
    near = run(*[t.cuda() for t in tok], {})
    for name in near:
        assert torch.equal(far[name], near[name]), name
    assert float(near["o"].float().abs().max()) > 0 and float(near["gk"].float().abs().max()) > 0


# ----------------------------------------------------------------------------------------------------------------- modules and model
@pytest.fixture(scope="module")
def fixture():
    return DO.load_fixture("deepseek_tiny")


@pytest.fixture(scope="module")
def mla_fixture():
    return DO.load_fixture("deepseek_mla")


def _model(t, **over):
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model

    torch.manual_seed(0)
    m = DeepSeekV3Model(dict(DO.TINY_DEEPSEEK, **over)).to(BF16)
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    if over.get("mtp_depth", 1) == 0:
        sd = {k: v for k, v in sd.items() if not k.startswith("mtp_modules.")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert set(missing) <= {"mask", "cos", "sin"} and not unexpected, (missing, unexpected)
    return m.cuda().train()


def _inputs(t, dev="cuda"):
    depth = DO.TINY_DEEPSEEK["mtp_depth"]
    return (t["in.ids"].to(dev), t["in.targets"].to(dev), [t[f"in.shifted_x.{k}"].to(dev) for k in range(depth)],
            [t[f"in.shifted_y.{k}"].to(dev) for k in range(depth)])


def test_multi_latent_attention_against_the_two_head_fixture(mla_fixture):
    from llm_quest_amd.common.buffers import GlobalBuffers
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_attention import MultiLatentAttention

    t, spec = mla_fixture, DO.MLA_FIXTURE
    att = MultiLatentAttention(spec["d_in"], spec["d_out"], spec["num_heads"]).to(BF16)
    att.load_state_dict({k[3:]: v for k, v in t.items() if k.startswith("sd.")})
    att = att.cuda().train()
    mask = GlobalBuffers.get_causal_mask(spec["context_length"]).cuda()
    cos, sin = [x.cuda() for x in GlobalBuffers.get_rope_params(spec["context_length"], spec["rope_base"], spec["d_out"] // spec["num_heads"] // 2)]
    x = t["in.x"].cuda().requires_grad_(True)
    y = att(x, mask, cos, sin)
    y.backward(t["in.dy"].cuda())
    bad = []
    judge("y", y, t["out.y"], t["twin.y"], bad)
    judge("dx", x.grad, t["out.dx"], t["twin.dx"], bad)
    params = dict(att.named_parameters())
    for n in ("wk_decoup.weight", "wk_decoup.bias", "wkv_down_proj.weight", "wkv_down_proj.bias"):
        judge("grad " + n, params[n].grad, t["out.grad." + n], t["twin.grad." + n], bad)
    for n, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    assert not bad, "\n".join(bad)


def test_model_against_the_reference_fixture(fixture):
    t = fixture
    m = _model(t)
    ids, tgt, sx, sy = _inputs(t)
    loss = m(ids, tgt, sx, sy)
    loss.backward()
    logits, h = m.main_model(ids, m.mask, m.cos, m.sin)
    assert logits.shape == t["out.logits"].shape and logits.dtype == BF16 and h.shape == (2, 70, DO.TINY_DEEPSEEK["emb_dim"])
    bad = []
    judge("loss", loss, t["out.loss"], t["twin.loss"], bad)
    judge("logits", logits, t["out.logits"], t["twin.logits"], bad)
    params = dict(m.named_parameters())
    judged, unjudged = 0, []
    for k in sorted(t):
        if not k.startswith("twin.grad."):
            continue
        name = k[len("twin.grad."):]
        g = params[name].grad
        assert g is not None and g.shape == params[name].shape and bool(torch.isfinite(g).all()), name
        if DO.rel_l2(t["grad." + name], t[k]) > 0.1:  # the reference's own floor: judged only where it is <= 0.1
            unjudged.append(name)
            continue
        judge("grad " + name, g, t["grad." + name], t[k], bad)
        judged += 1
    assert unjudged == ["main_model.trf_blocks.0.att.wk_up_proj.bias"] and judged == 29, (unjudged, judged)
    for name, p in params.items():  # the MTP block's output feeds nothing at mtp_depth = 1: no gradient, as in the reference
        if name.startswith("mtp_modules.0.trf_block."):
            assert "twin.grad." + name not in t and (p.grad is None or float(p.grad.float().abs().max()) == 0.0), name
    assert not bad, "\n".join(bad)


def test_kernels_on_the_captured_tensors_of_the_main_block(fixture):
    """The attention core of the reference's main block from its captured inputs (q and k as concatenated after RoPE, k repeated to the heads)
    through the kernels: the fixture's bf16 context as the reference flow, the fp64 restatement on the same inputs as the exact value."""
    t = fixture
    q, k, v, ctx = [t["cap.block0." + n] for n in ("q", "k", "v", "ctx")]
    B, H, S, Dn = v.shape
    Dr = q.shape[-1] - Dn
    assert (Dn, Dr) == (64, 32) and torch.equal(k[:, 0, :, Dn:], k[:, -1, :, Dn:])
    ops = (q[..., :Dn], q[..., Dn:], k[..., :Dn], k[:, 0, :, Dn:], v)
    dev = [DO.to_tokens(x).cuda() for x in ops[:3]] + [ops[3].reshape(B * S, Dr).contiguous().cuda(), DO.to_tokens(v).cuda()]
    o, _ = _km().mla_attn_fwd(*dev, B, S, H, Dn, Dr)
    bad = []
    judge("ctx", DO.from_tokens(o, B, S, H, Dn), ctx, DO.mla_attention(*ops, dtype=torch.float64)[0], bad)
    assert not bad, "\n".join(bad)


def test_twenty_optimizer_steps_lower_the_loss(fixture):
    from llm_quest_amd.optim import ArenaAdamW

    t = fixture
    m = _model(t)
    ids, tgt, sx, sy = _inputs(t)
    opt = ArenaAdamW(m.parameters(), lr=1e-3, weight_decay=0.0).attach(m)
    losses = []
    for step in range(21):
        loss = m(ids, tgt, sx, sy)
        losses.append(loss.detach())
        if step == 20:
            break
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if step == 0:
            arenas = m.arenas()
            assert len(arenas) == 3  # one MTP module, one main block, the shared top
            blk = m.main_model.trf_blocks[0]
            lo, hi = blk._arena.grad.data_ptr(), blk._arena.grad.data_ptr() + blk._arena.grad.numel() * 2
            for name, p in blk.named_parameters():
                assert p.grad is not None and lo <= p.grad.data_ptr() < hi and bool(torch.isfinite(p.grad).all()), name
        opt.step()
    first, last = float(losses[0]), float(losses[-1])
    print(f"  loss at step 0: {first:.4f}, at step 20: {last:.4f}")
    assert last == last and last < first


def test_eval_mode_and_depth_zero(fixture):
    t = fixture
    m = _model(t)
    ids, tgt, sx, sy = _inputs(t)
    with torch.no_grad():
        train_logits, _ = m.main_model(ids, m.mask, m.cos, m.sin)
        total = m(ids, tgt, sx, sy)
        m.eval()
        assert torch.equal(m(ids, None, None, None), train_logits)  # eval, y = None: the main logits
        main_only = m(ids, tgt, sx, sy)  # eval with targets: the main loss alone
    m0 = _model(t, mtp_depth=0)
    with torch.no_grad():
        depth0 = m0(ids, tgt, [], [])
    assert len(m0.mtp_modules) == 0 and float(depth0) == float(main_only)
    assert float(total) > float(main_only)  # the MTP term is a positive cross entropy
    ce = torch.nn.functional.cross_entropy(train_logits.float().flatten(0, 1), tgt.flatten())
    assert abs(float(ce) - float(main_only)) < 2e-2 * float(ce)


def test_modules_called_on_their_own(fixture):
    """SiLU, FFN, RMSNorm and MTPModule.forward outside the model: outputs and input gradients under the 1.5x rule, both flows of the restatement
    by autograd on the fixture's weights."""
    import torch.nn.functional as F

    from llm_quest_amd.llama3_to_deepseekv3 import deepseek_transformer_block as B

    t, cfg = fixture, DO.TINY_DEEPSEEK
    m = _model(t)
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    g = torch.Generator().manual_seed(77)
    rn = lambda *s, mul=1.0: (mul * torch.randn(*s, generator=g)).to(BF16)
    bad = []

    def both(fn, x, dy):
        out = {}
        for dt in (None, torch.float64):
            xg = DO._c(x, dt).detach().requires_grad_(True)
            y = fn(xg, dt)
            out[dt] = (y.detach(), torch.autograd.grad(y, xg, DO._c(dy, dt))[0])
        return out

    def mine(mod, x, dy):
        xg = x.cuda().requires_grad_(True)
        y = mod(xg)
        y.backward(dy.cuda())
        return y, xg.grad

    def check(name, got, flows):
        judge(name, got[0], flows[None][0], flows[torch.float64][0], bad)
        judge(name + " dx", got[1], flows[None][1], flows[torch.float64][1], bad)

    x, dy = rn(2, 70, 128, mul=3.0), rn(2, 70, 128)
    check("SiLU", mine(B.SiLU(), x, dy), both(lambda xg, dt: DO.silu(xg), x, dy))
    x, dy = rn(2, 70, cfg["emb_dim"]), rn(2, 70, cfg["emb_dim"])
    pf = "main_model.trf_blocks.0."
    w = lambda k, dt: DO._c(sd[pf + k], dt)
    ffn = lambda xg, dt: F.linear(F.linear(xg, w("ffn.lin1.weight", dt)) * DO.silu(F.linear(xg, w("ffn.lin_gate.weight", dt))), w("ffn.lin2.weight", dt))
    check("FFN", mine(m.main_model.trf_blocks[0].ffn, x, dy), both(ffn, x, dy))
    check("RMSNorm", mine(m.main_model.final_norm, x, dy), both(lambda xg, dt: DO.rmsnorm(xg, DO._c(sd["main_model.final_norm.scale"], dt)), x, dy))
    # MTPModule.forward: (logits from the down-projected input, h_curr)
    ids = t["in.shifted_x.0"]
    cos, sin = DO.tables(cfg)
    flows = {}
    for dt in (None, torch.float64):
        with torch.no_grad():
            logits, h_curr = DO.mtp_module(sd, "mtp_modules.0.", cfg, ids, x, cos, sin, dt)
        flows[dt] = (logits.detach(), h_curr.detach())
    hp = x.cuda()
    logits, h_curr = m.mtp_modules[0](ids.cuda(), hp, m.mask, m.cos, m.sin)
    judge("MTP logits", logits, flows[None][0], flows[torch.float64][0], bad)
    judge("MTP h_curr", h_curr, flows[None][1], flows[torch.float64][1], bad)
    assert not bad, "\n".join(bad)
