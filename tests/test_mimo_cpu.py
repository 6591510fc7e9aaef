"""MiMo-V2-Flash without a GPU: signatures and state_dict against the reference's, the layer pattern, the refusals, and the plain-torch
restatement (tests/mimo_oracle.py) against hand-checkable cases and against the reference fixture."""

import inspect
import json
import math
import os

import pytest
import torch

import gemma3_oracle as GO
import mimo_oracle as O

BF16 = torch.bfloat16
CFG = O.TINY_MIMO


def _mods():
    from llm_quest_amd.xiaomi import mimo_v2_flash_attention as A
    from llm_quest_amd.xiaomi import mimo_v2_flash_model as M
    from llm_quest_amd.xiaomi import mimo_v2_flash_transformer_block as B

    return A, B, M


def _sig():
    with open(os.path.join(O.GOLDEN, "mimo_signatures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    return O.load_fixture()


def test_constructor_and_forward_signatures_match_the_reference():
    A, B, M = _mods()
    sig = _sig()
    classes = dict(GroupedQueryAttentionWithSink=A.GroupedQueryAttentionWithSink, FFN=B.FFN, TransformerBlock=B.TransformerBlock, MTPModule=M.MTPModule,
                   MainModel=M.MainModel, MiMoModel=M.MiMoModel)
    assert set(sig["constructors"]) == set(classes)
    for name, cls in classes.items():
        params = {n: p for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"}
        assert list(params) == sig["constructors"][name], name
        defaults = {n: p.default for n, p in params.items() if p.default is not inspect.Parameter.empty}
        assert defaults == sig["constructor_defaults"][name], name
        # forward: the reference's names first, private extensions (leading underscore) only behind them
        fwd = [p for p in inspect.signature(cls.forward).parameters if p != "self"]
        public = [p for p in fwd if not p.startswith("_")]
        assert public == sig["forwards"][name] and fwd[: len(public)] == public, name


def test_state_dict_matches_the_reference_and_round_trips(fixture):
    _, _, M = _mods()
    sig = _sig()
    torch.manual_seed(0)
    m = M.MiMoModel(dict(CFG)).to(BF16)
    sd = m.state_dict()
    assert {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()} == sig["state_dict"]
    roots = {k.split(".")[1] if k.startswith("main_model.") else ".".join(k.split(".")[:3:2]) for k in sd}
    assert roots == {"emb_layer", "layers", "final_norm", "out_head", "mask_swa", "cos_swa", "sin_swa", "mask_ga", "cos_ga", "sin_ga", "mtp_modules.out_layer",
                     "mtp_modules.rms_h_prev", "mtp_modules.rms_input", "mtp_modules.final_norm", "mtp_modules.down_proj", "mtp_modules.trf_block"}
    att1 = {k.split(".")[4] for k in sd if k.startswith("main_model.layers.1.att.")}
    assert att1 == {"w_queries", "w_keys", "w_values", "out_proj", "q_norm", "k_norm", "sink"}
    assert not any(k.startswith("main_model.layers.0.att.sink") or k.startswith("main_model.layers.2.att.sink") for k in sd)  # GA layers have no sink
    assert m.mtp_modules[0].out_layer is m.main_model.out_head and m.mtp_modules[1].out_layer is m.main_model.out_head
    # the sink: upstream's shape and dtype; created in cfg["dtype"], N(0, 0.02)
    sink = M.MiMoModel(dict(CFG, dtype=torch.float32)).main_model.layers[1].att.sink.detach()
    assert sink.shape == (CFG["n_heads"],) and sink.dtype == torch.float32 and 0 < float(sink.abs().max()) < 0.2
    # the fixture's state loads (the config-derived buffers are not in it) and comes back bit for bit
    fsd = {k[3:]: v for k, v in fixture.items() if k.startswith("sd.")}
    res = m.load_state_dict(fsd, strict=False)
    assert not res.unexpected_keys and set(res.missing_keys) == {f"main_model.{a}_{b}" for a in ("mask", "cos", "sin") for b in ("swa", "ga")}
    back = m.state_dict()
    for k, v in fsd.items():
        assert torch.equal(back[k], v), k
    m2 = M.MiMoModel(dict(CFG)).to(BF16)
    m2.load_state_dict(back)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, back[k]), k
    # the tables: R = 20 of 64 (int(64 * 0.33) = 21, ten frequencies), two bases
    assert m.main_model.cos_swa.shape == (CFG["context_length"], 20) and not torch.equal(m.main_model.cos_swa, m.main_model.cos_ga)
    assert torch.equal(m.main_model.mask_swa, GO.band_mask(CFG["context_length"], CFG["window_size"]))
    assert torch.equal(m.main_model.mask_ga, GO.band_mask(CFG["context_length"], CFG["context_length"]))
    for swa, (c, s) in O.tables(CFG).items():
        mc, ms = (m.main_model.cos_swa, m.main_model.sin_swa) if swa else (m.main_model.cos_ga, m.main_model.sin_ga)
        assert torch.equal(c.to(BF16), mc) and torch.equal(s.to(BF16), ms)


@pytest.mark.parametrize("ratio,expect_swa", [
    (3, [False, True, False, True, True, False, True]),  # GA-dense, then SWA, GA, SWA, SWA, GA, SWA
    (6, [False, True, True, True, True, False, True]),  # the released 5 : 1 pattern
])
def test_layer_pattern(ratio, expect_swa):
    _, B, M = _mods()
    cfg = dict(CFG, n_layers=7, hybrid_ratio=ratio, num_experts=2, top_k=2, hidden_dim=8, vocab_size=16)
    main = M.MainModel(cfg)
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    assert [blk.use_sliding_window for blk in main.layers] == expect_swa == [O.is_swa(cfg, i) for i in range(7)]
    assert [blk.use_moe for blk in main.layers] == [False] + [True] * 6 == [O.is_moe(cfg, i) for i in range(7)]
    for i, blk in enumerate(main.layers):
        assert blk.layer_idx == i and isinstance(blk.feed_forward, DeepSeekMoE if i else B.FFN)
        assert blk.att.is_sliding_window == expect_swa[i] and hasattr(blk.att, "sink") == expect_swa[i]
        assert blk.att.num_kv_groups == (cfg["num_swa_kv_groups"] if expect_swa[i] else cfg["num_ga_kv_groups"])
        assert blk.window_size == (cfg["window_size"] if expect_swa[i] else None)
        assert blk.att.d_out == cfg["n_heads"] * cfg["value_head_dim"] and blk.att.out_proj.in_features == blk.att.d_out
        if i:
            assert blk.feed_forward.num_shared == 0 and not hasattr(blk.feed_forward, "shared_experts")


def test_value_head_dim_defaults_to_head_dim():
    A, _, _ = _mods()
    att = A.GroupedQueryAttentionWithSink(128, 4, 2, 64)
    assert att.value_head_dim == 64 and att.d_out == 256 and att.w_values.out_features == 128 and not att.is_sliding_window and not hasattr(att, "sink")
    att = A.GroupedQueryAttentionWithSink(128, 6, 2, 128, value_head_dim=64, is_sliding_window=True, dtype=BF16)
    assert att.d_out == 384 and att.w_keys.out_features == 256 and att.w_values.out_features == 128 and att.sink.dtype == BF16 and att.num_repeat == 3


def test_refusals():
    A, B, M = _mods()
    from llm_quest_amd import kernels_mimo as KM
    from llm_quest_amd import ops_g3, ops_mimo

    ids = torch.zeros(2, 8, dtype=torch.long)
    m = M.MiMoModel(dict(CFG)).to(BF16)
    main = m.main_model
    x = torch.zeros(2, 8, 128, dtype=BF16)
    # no CPU fallback, at every level
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(ids, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        main(ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        main.layers[1](x, main.mask_swa, main.cos_swa, main.sin_swa)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        main.layers[1].att(x, main.mask_swa, main.cos_swa, main.sin_swa)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        main.layers[0].feed_forward(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.sink_attn_fwd(x[0], x[0], x[0], 1, 8, 2, 2, 64, 64, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.normrope_fwd(x[0], 8, 1, 1, 64, main.cos_swa.float(), main.sin_swa.float(), main.layers[1].att.q_norm.weight, main.layers[1].att.k_norm.weight)
    # a padding mask
    am = torch.ones(2, 8, dtype=torch.bool)
    for call in (lambda: main(ids, am), lambda: main.layers[1](x, main.mask_swa, main.cos_swa, main.sin_swa, am),
                 lambda: main.layers[1].att(x, main.mask_swa, main.cos_swa, main.sin_swa, attn_mask=am)):
        if torch.cuda.is_available():
            with pytest.raises(NotImplementedError, match="attn_mask"):
                call()
    with pytest.raises(NotImplementedError, match="attn_mask"):
        ops_mimo.refuse_attn_mask(am, "MainModel")
    assert "attn_mask" not in inspect.signature(M.MiMoModel.forward).parameters  # the model never passes one upstream
    # an unbuilt (head_dim, value_head_dim), refused by name when the module is built
    for D, DV in ((96, 32), (64, 128), (128, 32), (256, 128)):
        with pytest.raises(ValueError, match=rf"\({D}, {DV}\) not built"):
            A.GroupedQueryAttentionWithSink(128, 4, 2, D, value_head_dim=DV)
        with pytest.raises(ValueError, match="not built"):
            M.MiMoModel(dict(CFG, head_dim=D, value_head_dim=DV))
    for D, DV in KM.HEAD_DIM_PAIRS:
        A.GroupedQueryAttentionWithSink(64, 2, 1, D, value_head_dim=DV)
    assert (192, 128) in KM.HEAD_DIM_PAIRS  # the released model's pair
    # a non-bf16 model, S > context_length, a window below 1, a mask that is no band: checked before anything reaches a kernel
    with pytest.raises(TypeError, match=r"to\(torch.bfloat16\)"):
        ops_g3.check_bf16(M.MiMoModel(dict(CFG, dtype=torch.float32)), "MiMoModel")
    with pytest.raises(ValueError, match="exceeds context_length"):
        ops_mimo.make_runtime(main, 1, 97, CFG["window_size"], main.cos_swa, main.sin_swa, CFG["context_length"])
    with pytest.raises(ValueError, match="exceeds context_length"):
        ops_mimo.make_runtime(main, 1, 50, 24, main.cos_swa[:40], main.sin_swa[:40])
    with pytest.raises(ValueError, match="at least 1"):
        ops_mimo.make_runtime(main, 1, 8, 0, main.cos_swa, main.sin_swa)
    assert ops_mimo.window_of(main.mask_swa, 70) == 24 and ops_mimo.window_of(main.mask_ga, 70) == 70 and ops_mimo.window_of(main.mask_swa, 10) == 10
    with pytest.raises(ValueError, match="sliding-window band"):
        ops_mimo.window_of(~main.mask_ga, 8)
    edited = main.mask_ga.clone()
    assert ops_mimo.window_of(edited, 8) == 8
    edited[7, 0] = True  # an in-place edit is seen: the remembered window belongs to one version of one tensor
    assert ops_mimo.window_of(edited, 8) == 7
    edited[5, 2] = True
    with pytest.raises(ValueError, match="sliding-window band"):
        ops_mimo.window_of(edited, 8)
    for i in range(1, 8):
        edited[i, :i] = True
    assert ops_mimo.window_of(edited, 8) == 1
    if torch.cuda.is_available():
        with pytest.raises(TypeError, match=r"to\(torch.bfloat16\)"):
            M.MiMoModel(dict(CFG, dtype=torch.float32)).cuda()(ids.cuda(), ids.cuda())
        mc = m.cuda()
        with pytest.raises(ValueError, match="exceeds context_length"):
            mc(torch.zeros(1, 97, dtype=torch.long, device="cuda"), torch.zeros(1, 97, dtype=torch.long, device="cuda"))
        with pytest.raises(ValueError, match="targets must be provided"):
            mc.train()(ids.cuda())


def test_launchers_refuse_bad_arguments_before_a_launch():
    """The host checks of kernels_mimo run before ``require_gpu`` would matter only on a device; here they are reached through the library's C entry
    points, which validate without touching a GPU, and return a code plus a message."""
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    q = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first
    fwd = lambda B=1, S=8, Hq=6, Hkv=2, D=64, DV=32, W=4, ptr=q, ldq=384, ldk=128, ldv=64, ldo=192: lib.mi355_sink_attn_fwd(
        B, S, Hq, Hkv, D, DV, W, ptr, ldq, q, ldk, q, ldv, None, q, ldo, q, 0.125, None)
    bwd = lambda parts=1, sink=q, part=q, lddv=64, dq=q: lib.mi355_sink_attn_bwd(1, 8, 6, 2, 64, 32, 4, q, 384, q, 128, q, 64, q, 192, q, 192, sink, q, q, dq, 384, q, 128, q, lddv,
                                                                                  part, parts, 0.125, None)
    nr = lambda D=64, R=20, ldx=512, rows=8, x=q, Hq=6: lib.mi355_mimo_normrope_fwd(8, 8, Hq, 2, D, R, x, ldx, q, q, q, q, rows, q, 512, 1e-6, None)
    nrb = lambda parts=4, ldd=512, R=20: lib.mi355_mimo_normrope_bwd(8, 8, 6, 2, 64, R, q, 512, q, q, q, q, 8, q, 512, q, ldd, q, parts, 1e-6, None)
    cases = [
        (lambda: fwd(ptr=None), b"null pointer"), (lambda: fwd(D=96), b"(96, 32) not built"), (lambda: fwd(D=64, DV=128), b"(64, 128) not built"),
        (lambda: fwd(W=0), b"window 0 must be at least 1"), (lambda: fwd(Hq=5), b"must be a multiple of kv heads"), (lambda: fwd(ldq=383), b"leading dimension"),
        (lambda: fwd(ldv=60), b"leading dimension"), (lambda: fwd(ldo=196), b"multiples of 8"), (lambda: fwd(S=-1), b"negative batch or sequence"),
        (lambda: fwd(S=(1 << 30) - 32), b"grid limits"), (lambda: fwd(B=70000), b"grid limits"), (lambda: fwd(ptr=q + 2), b"16-byte aligned"),
        (lambda: bwd(parts=0), b"parts in 1..65535"), (lambda: bwd(part=None), b"dsink_partial must be given"), (lambda: bwd(lddv=56), b"leading dimension"),
        (lambda: bwd(dq=None), b"null pointer"),
        (lambda: nr(D=32), b"head_dim 32 not built"), (lambda: nr(R=21), b"must be even"), (lambda: nr(R=66), b"must be even and in [2, head_dim = 64]"),
        (lambda: nr(R=0), b"must be even"), (lambda: nr(ldx=500), b"leading dimension"), (lambda: nr(rows=7), b"coefficient table has 7 rows"),
        (lambda: nr(x=None), b"null pointer"), (lambda: nr(Hq=-1), b"bad token / head counts"),
        (lambda: nrb(parts=0), b"parts in 1..65535"), (lambda: nrb(ldd=384), b"leading dimension"), (lambda: nrb(R=22 + 1), b"must be even"),
    ]
    for call, msg in cases:
        rc = call()
        assert rc != 0 and msg in lib.mi355_last_error(), (msg, lib.mi355_last_error())
    assert fwd(B=0) == 0 and fwd(S=0) == 0  # empty problems


# ----------------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_without_a_sink_is_the_windowed_attention_oracle():
    q, k, v, do, _ = O.attn_operands(2, 37, 6, 2, 64, 64, seed=1, sink=False)
    neg = torch.full((6,), -math.inf)
    for W in (1, 5, 37, 100):
        for exact in (False, True):
            o, lse = GO.swa_attention(q, k, v, W, exact)
            for sink in (None, neg.to(BF16) if not exact else neg.double()):
                o2, lse2 = O.sink_attention(q, k, v, W, sink, exact)
                assert torch.equal(o, o2) and torch.equal(lse, lse2)
            for a, b in zip(GO.swa_attention_bwd(q, k, v, do, W, exact), O.sink_attention_bwd(q, k, v, do, W, None, exact)[:3]):
                assert torch.equal(a, b)


def test_oracle_with_one_key_scales_the_value():
    """W = 1: the softmax holds the key itself and the sink, so o = v / (1 + exp(z - s)) and lse = log(exp(s) + exp(z))."""
    q, k, v, _, z = O.attn_operands(2, 9, 3, 3, 64, 32, seed=2)
    o, lse = O.sink_attention(q, k, v, 1, z, True)
    s = (q.double() * k.double()).sum(-1) * 64 ** -0.5
    zz = z.double().view(1, 3, 1)
    assert torch.allclose(o, v.double() / (1 + torch.exp(zz - s)).unsqueeze(-1), rtol=1e-12, atol=1e-14)
    assert torch.allclose(lse, torch.log(torch.exp(s) + torch.exp(zz)), rtol=1e-12, atol=1e-14)
    # the sink is not multiplied by the scale: with q = 0 every score is 0 and p_sink = e^z / (n + e^z)
    o0, _ = O.sink_attention(torch.zeros_like(q), k, torch.ones_like(v), 4, z, True)
    n = torch.arange(1, 10).clamp(max=4).double().view(1, 1, 9, 1)
    assert torch.allclose(o0, (n / (n + torch.exp(zz.unsqueeze(-1)))).expand_as(o0), rtol=1e-12)


def test_oracle_sink_gradient_formula_against_autograd():
    """dz[h] = - sum_{b,i} exp(z_h - lse[b,h,i]) delta[b,h,i] with delta = rowsum(dO * O), in fp64; and delta / dS as the kernels form them."""
    for (B, S, Hq, Hkv, D, DV, W) in ((2, 23, 6, 2, 64, 32, 5), (1, 40, 6, 1, 64, 64, 40)):
        q, k, v, do, z = O.attn_operands(B, S, Hq, Hkv, D, DV, seed=3 + S)
        o, lse = O.sink_attention(q, k, v, W, z, True)
        dq, dk, dv, dz = O.sink_attention_bwd(q, k, v, do, W, z, True)
        delta = (do.double() * o).sum(-1)
        assert torch.allclose(O.dsink_formula(z.double(), lse, delta), dz, rtol=1e-10, atol=1e-13)
        # dq from p recomputed out of lse (sink included) and dS = p (dP - delta)
        rep = Hq // Hkv
        kk, vv = k.double().repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1)
        sc = (q.double() @ kk.mT) * D ** -0.5
        p = torch.exp(sc - lse.unsqueeze(-1)).masked_fill(GO.band_mask(S, W), 0.0)
        ds = p * (do.double() @ vv.mT - delta.unsqueeze(-1))
        assert torch.allclose(ds @ kk * D ** -0.5, dq, rtol=1e-9, atol=1e-12)
        assert float(p.sum(-1).max()) < 1.0  # the sink holds the rest of every row


def test_oracle_flows_agree_and_norm_rope_passes_the_tail_through():
    q, k, v, do, z = O.attn_operands(2, 37, 6, 2, 64, 32, seed=4)
    for W in (1, 5, 100):
        a, b = O.sink_attention(q, k, v, W, z), O.sink_attention(q, k, v, W, z, True)
        assert O.rel_l2(a[0], b[0]) < 1e-2 and O.rel_l2(a[1], b[1]) < 1e-2
        for g, e in zip(O.sink_attention_bwd(q, k, v, do, W, z), O.sink_attention_bwd(q, k, v, do, W, z, True)):
            assert g.shape == e.shape and O.rel_l2(g, e) < 5e-2
    x, dy, w = O.norm_rope_operands(2, 9, 3, 64, seed=5)
    cos, sin = O.rope_tables(10000, 64, 16, 0.33)
    assert cos.shape == (16, 20)
    for exact in (False, True):
        y = O.norm_rope(x, w, cos, sin, exact)
        assert torch.equal(y[..., 20:], O.rms_norm(O._c(x, exact), O._c(w, exact), exact)[..., 20:])  # features >= R: the norm alone
        assert torch.equal(y[:, :, 0], O.rms_norm(O._c(x, exact), O._c(w, exact), exact)[:, :, 0].to(y.dtype))  # position 0: cos = 1, sin = 0
    assert O.rel_l2(O.norm_rope(x, w, cos, sin), O.norm_rope(x, w, cos, sin, True)) < 1e-2
    for g, e in zip(O.norm_rope_bwd(x, w, cos, sin, dy), O.norm_rope_bwd(x, w, cos, sin, dy, True)):
        assert O.rel_l2(g, e) < 2e-2
    # the rotation pairs are (d, d + R/2): a unit vector at feature 3 moves into features 3 and 13 only
    e3 = torch.zeros(1, 1, 4, 64, dtype=torch.float64)
    e3[..., 3] = 1
    r = O.partial_rope(e3, cos, sin, True)
    assert set(torch.nonzero(r[0, 0, 2]).flatten().tolist()) == {3, 13}


def test_oracle_model_reproduces_the_reference_fixture(fixture):
    """The restatement in the reference's dtype flow, fed the fixture's weights, inputs and selection, against the reference's own logits and loss; and
    its fp64 flow against the fp32 twin.  Per MoE layer the recorded selection, counts and updated biases are the fixture's."""
    t = fixture
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    idxs = {i: t[f"moe.{i}.topk_idxs"].long() for i in O.moe_layers(CFG)}
    rec = {}
    loss, logits = O.model_loss(sd, CFG, t["in.ids"], t["in.targets"], False, idxs, rec)
    assert O.rel_l2(logits, t["out.logits"]) < 2e-2 and abs(float(loss) - float(t["out.loss"])) < 0.05
    for i in O.moe_layers(CFG):
        assert torch.equal(rec[i]["counts"].int(), t[f"moe.{i}.counts"]) and torch.equal(rec[i]["biases"], t[f"moe.{i}.biases"])
    loss64, logits64 = O.model_loss(sd, CFG, t["in.ids"], t["in.targets"], True, idxs)
    assert O.rel_l2(logits64, t["twin.logits"]) < 1e-4 and abs(float(loss64) - float(t["twin.loss"])) < 1e-4
    caps = {}
    O.main_model(sd, CFG, t["in.ids"], True, idxs, None, caps)
    for i in (1, 2):
        for name in ("q", "k", "v", "ctx"):
            assert caps[i][name].shape == t[f"cap.{i}.{name}"].shape and O.rel_l2(t[f"cap.{i}.{name}"], caps[i][name]) < 3e-2, (i, name)


def test_fixture_meets_its_stated_conditions(fixture):
    import deepseek_moe_oracle as MO

    t, sig = fixture, _sig()
    files = [f for f in os.listdir(O.GOLDEN) if f.startswith("mimo_tiny") and f.endswith(".safetensors")]
    assert 1 <= len(files) <= 12 and all(os.path.getsize(os.path.join(O.GOLDEN, f)) < (1 << 20) for f in files)
    assert t["in.ids"].shape == (O.FIXTURE_BATCH, O.FIXTURE_SEQ) and bool((t["in.targets"] == -100).any())
    names = [k[5:] for k in t if k.startswith("grad.")]
    assert set(names) == {k[10:] for k in t if k.startswith("twin.grad.")} == set(sig["floors"])
    params = {k[3:] for k in t if k.startswith("sd.") and t[k].is_floating_point() and not k.endswith(".biases") and ".out_layer." not in k}
    assert set(names) == params  # every parameter received a gradient in the reference
    above = 0
    for n in names:
        floor = O.rel_l2(t["grad." + n], t["twin.grad." + n])
        assert abs(floor - sig["floors"][n]) <= 1e-3 * floor + 1e-12, n
        above += floor > 0.1
        assert floor <= 0.1 or O.floor_allowed(n), n
    assert above * 10 <= len(names)
    for i in O.moe_layers(CFG):
        pre = f"moe.{i}."
        b0 = t[f"sd.main_model.layers.{i}.feed_forward.biases"]
        assert float(b0.abs().min()) > 0  # non-zero before the forward
        assert int(MO.key_boundary_tie(t[pre + "logits"], b0, CFG["top_k"]).sum()) == 0
        p = torch.softmax(t[pre + "logits"], dim=-1)
        plain = p.topk(CFG["top_k"], dim=-1)[1].sort(dim=1).values
        assert bool((plain != t[pre + "topk_idxs"].long().sort(dim=1).values).any())
        assert torch.equal(t[pre + "robust"].bool(), MO.robust_tokens(t[pre + "logits"], b0, CFG["top_k"]))
    first = t[f"moe.{O.moe_layers(CFG)[0]}.robust"]
    assert int(first.sum()) * 10 >= 9 * first.numel()
