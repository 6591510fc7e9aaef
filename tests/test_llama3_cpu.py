"""Llama 3.2 and QK-Clip without a GPU: signatures and configs against the reference's, the plain-torch restatement (tests/llama3_oracle.py) against
the reference fixture (logits, loss, gradients, per-head maximum logits, the three clipped weight sets), the refusals, the host-side validation of
the new entry points, and the fixture's own floor condition."""

import ctypes
import inspect
import json
import os

import pytest
import torch

import llama3_oracle as LO

BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = LO.TINY_LLAMA
HQ, HKV = CFG["n_heads"], CFG["num_kv_groups"]


def _mods():
    from llm_quest_amd.gpt_to_llama3 import llama_attention as A
    from llm_quest_amd.gpt_to_llama3 import llama_model as M
    from llm_quest_amd.gpt_to_llama3 import llama_transformer_block as B

    return A, B, M


@pytest.fixture(scope="module")
def fixture():
    return LO.load_fixture("llama3_tiny")


@pytest.fixture(scope="module")
def sig():
    return json.load(open(os.path.join(GOLDEN, "llama3_signatures.json")))


def close(a, b, rtol=0.0, atol=0.0):
    torch.testing.assert_close(a.float(), b.float(), rtol=rtol, atol=atol)


# ----------------------------------------------------------------------------------------------------------------- signatures
def test_signatures_and_state_dict_match_the_reference(sig):
    A, B, M = _mods()
    from llm_quest_amd.common import qk_clip as QC

    classes = dict(GroupedQueryAttention=A.GroupedQueryAttention, RMSNorm=B.RMSNorm, SiLU=B.SiLU, FFN=B.FFN, TransformerBlock=B.TransformerBlock,
                   Llama3Model=M.Llama3Model, QKClipNaive=QC.QKClipNaive, QKClip=QC.QKClip, MagnitudeQKClipMHA=QC.MagnitudeQKClipMHA)
    assert set(sig["constructors"]) == set(classes)
    params = lambda fn: [p for p in inspect.signature(fn).parameters if p != "self"]
    for name, cls in classes.items():
        assert params(cls.__init__) == sig["constructors"][name], name
    # forward signatures: the reference's names first, private extensions (leading underscore) only behind them
    for name, want in sig["forwards"].items():
        assert [p for p in params(classes[name].forward) if not p.startswith("_")] == want, name
    for name, want in sig["calls"].items():
        assert params(classes[name].__call__) == want, name
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    m = M.Llama3Model(dict(CFG)).to(BF16)
    assert desc(m.state_dict()) == sig["state_dict"]
    assert m.out_head.weight is m.emb_dict.weight  # tied, as upstream
    att = m.trf_blocks[0].att
    assert att.track_max_attn_logit is False and att.max_attn_logit is None
    assert (att.num_heads, att.num_kv_groups, att.num_repeat, att.head_dim, att.att_scaling) == (4, 2, 2, 64, 0.125)
    assert m.cos.shape == (CFG["context_length"], 64) and m.mask.dtype == torch.bool


def test_configs_match_the_reference(sig):
    from llm_quest_amd import config

    for name, want in sig["configs"].items():
        got = dict(getattr(config, name))
        dtype = got.pop("dtype")
        assert got == want, name
        assert dtype == (torch.bfloat16 if name.endswith("_1B") else torch.float32)


# ----------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_reproduces_the_model_fixture(fixture):
    """Same ops in the same dtype flow: logits and loss bit for bit, gradients to the tolerances of test_oracle_golden.py::test_qwen3_tiny."""
    t = fixture
    sd = LO.state_dict_of(t)
    km = t["in.key_mask"]
    cap = []
    logits = LO.model(sd, CFG, t["in.ids"], km, capture=cap)
    assert logits.dtype == BF16 and torch.equal(logits, t["out.logits"])
    assert torch.equal(LO.model(sd, CFG, t["in.ids"]), t["out.logits_nomask"])
    loss, _, grads = LO.model_grads(sd, CFG, t["in.ids"], t["in.targets"], km)
    assert torch.equal(loss, t["out.loss"])
    names = [k[5:] for k in t if k.startswith("grad.")]
    assert len(names) == 22 and set(names) == set(grads)
    for n in names:
        close(grads[n], t["grad." + n], rtol=1e-2, atol=1e-3)
    # the oracle's maximum logits are the fixture's (the softmax input's amax over batch, query and key)
    for i in range(CFG["n_layers"]):
        assert torch.equal(cap[i].float(), t[f"out.max_logits.{i}"]), i
    cap = []
    LO.model(sd, CFG, t["in.ids"], capture=cap)
    for i in range(CFG["n_layers"]):
        assert torch.equal(cap[i].float(), t[f"out.max_logits_nomask.{i}"]), i


def test_restatement_matches_the_twin(fixture):
    t = fixture
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in LO.state_dict_of(t).items()}
    loss, logits, grads = LO.model_grads(sd32, CFG, t["in.ids"], t["in.targets"], t["in.key_mask"])
    close(logits, t["twin.logits"], atol=1e-5)
    assert abs(float(loss) - float(t["twin.loss"])) / float(t["twin.loss"]) < 1e-5
    for n, g in grads.items():
        assert LO.rel_l2(g, t["twin.grad." + n]) < 1e-4, n
    # the fp64 flow on the bf16 weights agrees with the twin to fp32 rounding
    l64, _ = LO.model_loss(LO.state_dict_of(t), CFG, t["in.ids"], t["in.targets"], t["in.key_mask"], exact=True)
    assert l64.dtype == torch.float64 and abs(float(l64) - float(t["twin.loss"])) / float(t["twin.loss"]) < 1e-5


def test_max_logit_restatement_on_model_operands(fixture):
    """``max_logit`` on the q, k the restatement's first layer holds gives that layer's recorded maximum, in both mask settings; the fp64 value lies
    within the bf16 rounding of a score."""
    t = fixture
    sd = LO.state_dict_of(t)
    cos, sin = LO.tables(CFG)
    x = LO.rmsnorm(torch.nn.functional.embedding(t["in.ids"], sd["emb_dict.weight"]), sd["trf_blocks.0.norm_1.scale"])
    b, s, _ = x.shape
    q = LO.rope(torch.nn.functional.linear(x, sd["trf_blocks.0.att.w_queries.weight"]).view(b, s, HQ, 64).transpose(1, 2), cos, sin)
    k = LO.rope(torch.nn.functional.linear(x, sd["trf_blocks.0.att.w_keys.weight"]).view(b, s, HKV, 64).transpose(1, 2), cos, sin)
    assert torch.equal(LO.max_logit(q, k, key_mask=t["in.key_mask"]).float(), t["out.max_logits.0"])
    assert torch.equal(LO.max_logit(q, k).float(), t["out.max_logits_nomask.0"])
    m64 = LO.max_logit(q, k, key_mask=t["in.key_mask"], exact=True)
    assert m64.dtype == torch.float64 and LO.rel_l2(m64, t["out.max_logits.0"]) < 2.0 ** -7
    # the packed-projection form is the per-tensor form
    qkv = torch.cat((LO.to_tokens(q), LO.to_tokens(k), LO.to_tokens(k)), dim=1)
    pos = torch.arange(s, dtype=torch.int32).repeat(b)
    q2, k2 = LO.rope_packed_fwd(qkv, cos, sin, pos, b, s, HQ, HKV, 64)
    assert torch.equal(q2, LO.to_tokens(LO.rope(q, cos, sin))) and torch.equal(k2, LO.to_tokens(LO.rope(k, cos, sin)))


def _check_clip(before_q, before_k, got, want_q, want_k, Hq, Hkv):
    """Bit for bit on the heads upstream left alone, within one bf16 step elsewhere."""
    bad = LO.clip_mismatches(before_q, got[0], want_q, Hq) + LO.clip_mismatches(before_k, got[1], want_k, Hkv)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", ["per_head", "naive"])
def test_clip_restatement_reproduces_the_fixture(fixture, mode):
    t = fixture
    touched = 0
    for i in range(CFG["n_layers"]):
        pq, pk = f"trf_blocks.{i}.att.w_queries.weight", f"trf_blocks.{i}.att.w_keys.weight"
        got = LO.qk_clip(t["sd." + pq], t["sd." + pk], t[f"out.max_logits.{i}"], HQ, HKV, LO.FIXTURE_TAU, 0.5, mode)
        _check_clip(t["sd." + pq], t["sd." + pk], got, t[f"clip.{mode}.{pq}"], t[f"clip.{mode}.{pk}"], HQ, HKV)
        touched += not torch.equal(t[f"clip.{mode}.{pq}"], t["sd." + pq])
    assert touched >= 1
    if mode == "per_head":  # a head at exactly the threshold is not clipped, its neighbours are
        m0 = t["out.max_logits.0"]
        assert (m0 == LO.FIXTURE_TAU).any() and (m0 > LO.FIXTURE_TAU).any()


def test_magnitude_clip_restatement_reproduces_the_fixture(fixture):
    t = fixture
    for i in range(CFG["n_layers"]):
        pq, pk = f"trf_blocks.{i}.att.w_queries.weight", f"trf_blocks.{i}.att.w_keys.weight"
        got = LO.qk_clip(t["mha.sd." + pq], t["mha.sd." + pk], t[f"mha.max_logits.{i}"], HQ, HQ, LO.FIXTURE_TAU, 0.5, "magnitude")
        _check_clip(t["mha.sd." + pq], t["mha.sd." + pk], got, t["mha.clip.magnitude." + pq], t["mha.clip.magnitude." + pk], HQ, HQ)
    with pytest.raises(ValueError, match="multi-head attention only"):
        LO.qk_clip(t["sd.trf_blocks.0.att.w_queries.weight"], t["sd.trf_blocks.0.att.w_keys.weight"], t["out.max_logits.0"], HQ, HKV, 4.0, 0.5, "magnitude")


def test_clip_restatement_never_clips_on_degenerate_maxima():
    w = torch.randn(4 * 8, 16).to(BF16)
    wk = torch.randn(2 * 8, 16).to(BF16)
    m = torch.tensor([float("nan"), -float("inf"), -5.0, 4.0])
    for mode in ("per_head", "naive"):
        q2, k2 = LO.qk_clip(w, wk, m, 4, 2, 4.0, 0.5, mode)
        assert torch.equal(q2, w) and torch.equal(k2, wk), mode
    # the group's minimum gamma: only head 1 of group 0 exceeds the threshold, the group's key head follows it
    m = torch.tensor([1.0, 16.0, 2.0, 3.0])
    q2, k2 = LO.qk_clip(w, wk, m, 4, 2, 4.0, 0.5, "per_head")
    assert torch.equal(q2[:8], w[:8]) and torch.equal(q2[16:], w[16:]) and torch.equal(k2[8:], wk[8:])
    assert torch.equal(q2[8:16], (w[8:16].float() * 0.5).to(BF16)) and torch.equal(k2[:8], (wk[:8].float() * 0.5).to(BF16))


def test_fixture_floors_meet_the_condition(fixture, sig):
    """The premise of the model test: the reference's own bf16-vs-twin distance is <= 0.1 on EVERY gradient tensor (no tensor is excluded)."""
    t = fixture
    names = [k[10:] for k in t if k.startswith("twin.grad.")]
    assert len(names) == 22 and set(sig["floors"]) == set(names)
    for n in names:
        assert LO.rel_l2(t["grad." + n], t["twin.grad." + n]) <= 0.1, n
    assert (t["in.key_mask"][1, -4:] == 0).all() and int(t["in.key_mask"].sum()) == 2 * 24 - 4


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    A, B, M = _mods()
    from llm_quest_amd import kernels_llama as KL
    from llm_quest_amd import ops_llama
    from llm_quest_amd.common import qk_clip as QC

    with pytest.raises(ValueError, match="head_dim 32 not built"):
        A.GroupedQueryAttention(64, 64, 2, 1)
    with pytest.raises(ValueError, match="head_dim 32 not built"):
        M.Llama3Model(dict(CFG, emb_dim=128))
    m = M.Llama3Model(dict(CFG)).to(BF16)
    ids = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(ids)
    x = torch.zeros(2, 8, CFG["emb_dim"], dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.trf_blocks[0](x, m.mask, m.cos, m.sin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.trf_blocks[0].att(x, m.mask, m.cos, m.sin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.final_norm(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.trf_blocks[0].ffn(x)
    with pytest.raises(TypeError, match=r"to\(torch.bfloat16\)"):
        ops_llama.check_bf16(M.Llama3Model(dict(CFG)), "Llama3Model")  # the norm scales are still fp32
    with pytest.raises(TypeError, match=r"to\(torch.bfloat16\)"):
        ops_llama.check_bf16(M.Llama3Model(dict(CFG, dtype=torch.float32)), "Llama3Model")
    z = lambda r, w: torch.zeros(r, w, dtype=BF16)
    tab = torch.zeros(8, 64)
    pos = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.rope_fwd(z(8, 256), tab, tab, pos, 2, 1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.rope_bwd(z(8, 128), z(8, 64), tab, tab, pos, z(8, 256), 2, 1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.attn_max_logit(z(8, 128), z(8, 64), 1, 8, 2, 1, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.qk_clip_(z(128, 32), z(64, 32), torch.zeros(2), 2, 1, 4.0)
    # QK-Clip on the model: nothing tracked yet; the magnitude variant refuses a GQA model before it touches a weight
    with pytest.raises(RuntimeError, match="track_max_attn_logit"):
        QC.collect_max_attn_logits(m)
    with pytest.raises(ValueError, match="multi-head attention only"):
        QC.MagnitudeQKClipMHA(4.0)(m, [torch.zeros(4), torch.zeros(4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QC.QKClip(4.0)(m, [torch.zeros(4), torch.zeros(4)])
    clip = QC.QKClip(100, alpha=0.3)
    assert (clip.clip_threshold, clip.alpha) == (100, 0.3)


# ----------------------------------------------------------------------------------------------------------------- host-side validation
def _lib_and_buffer():
    from llm_quest_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(8192 + 16)
    return lib, buf, (ctypes.addressof(buf) + 15) & ~15


def _refused(lib, name, args, expect):
    rc = getattr(lib, name)(*args)
    msg = lib.mi355_last_error().decode()
    assert rc != 0 and msg and expect in msg, (name, rc, msg)


def test_entry_points_refuse_bad_calls_with_a_message():
    """No kernel is ever launched by these calls: each is refused by the validation first."""
    lib, _keep, p = _lib_and_buffer()
    M, Hq, Hkv, D = 8, 2, 1, 64
    fwd = [M, Hq, Hkv, D, p, (Hq + 2 * Hkv) * D, p, p, 8, p, p, p, None]
    bwd = [M, Hq, Hkv, D, p, Hq * D, p, Hkv * D, p, p, 8, p, p, (Hq + 2 * Hkv) * D, None]
    mx = [1, 8, Hq, Hkv, D, p, Hq * D, p, Hkv * D, None, 0.125, p, 2, p, None]
    clip = [Hq, Hkv, D, 32, p, p, p, 4.0, 0.5, 0, None]
    for name, good, d_at, ptr_at, ld_at in (("mi355_llama_rope_fwd", fwd, 3, 4, 5), ("mi355_llama_rope_bwd", bwd, 3, 4, 5), ("mi355_attn_max_logit", mx, 4, 5, 6)):
        bad = list(good)
        bad[d_at] = 32
        _refused(lib, name, bad, "not built")
        bad = list(good)
        bad[ptr_at] = None
        _refused(lib, name, bad, "null pointer")
        bad = list(good)
        bad[ptr_at] = p + 2
        _refused(lib, name, bad, "16-byte aligned")
        bad = list(good)
        bad[ld_at] = 8
        _refused(lib, name, bad, "at least" if name.endswith("rope_fwd") else "leading dimension")
        bad = list(good)
        bad[2 if name != "mi355_attn_max_logit" else 3] = 3  # kv heads that do not divide the query heads
        _refused(lib, name, bad, "multiple of kv heads")
    bad = list(mx)
    bad[12] = 1  # partial buffer too small: B * ceil(S / 128) * Hq = 2 floats needed
    _refused(lib, "mi355_attn_max_logit", bad, "partial holds")
    assert lib.mi355_attn_max_logit_partials(2, 129, 4) == 4 * 2 * 2 and lib.mi355_attn_max_logit_partials(2, 128, 4) == 8
    assert lib.mi355_attn_max_logit_partials(0, 128, 4) == 0
    assert lib.mi355_llama_rope_fwd(0, Hq, Hkv, D, None, 0, None, None, 0, None, None, None, None) == 0  # no tokens: an empty problem
    for at, val, expect in ((9, 3, "mode 3"), (7, 0.0, "threshold must be positive"), (8, 1.5, "alpha in [0, 1]"), (4, None, "null pointer"), (1, 3, "multiple of kv heads")):
        bad = list(clip)
        bad[at] = val
        _refused(lib, "mi355_qk_clip", bad, expect)
    _refused(lib, "mi355_qk_clip", [Hq, Hkv, D, 32, p, p, p, 4.0, 0.5, 2, None], "multi-head attention only")
