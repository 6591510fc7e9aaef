"""DeepSeek-V3 dense path without a GPU: the plain-torch restatement (tests/deepseek_oracle.py) against both reference fixtures, signatures
against the reference's, the refusals, the host-side validation of the four MLA entry points, and the fixture's own floor condition."""

import ctypes
import inspect
import json
import os

import pytest
import torch

import deepseek_oracle as DO

BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = DO.TINY_DEEPSEEK


def _mods():
    from llm_quest_amd.llama3_to_deepseekv3 import deepseek_attention as A
    from llm_quest_amd.llama3_to_deepseekv3 import deepseek_model as M
    from llm_quest_amd.llama3_to_deepseekv3 import deepseek_transformer_block as B

    return A, B, M


@pytest.fixture(scope="module")
def fixture():
    return DO.load_fixture("deepseek_tiny")


@pytest.fixture(scope="module")
def mla_fixture():
    return DO.load_fixture("deepseek_mla")


def _inputs(t):
    depth = CFG["mtp_depth"]
    return t["in.ids"], t["in.targets"], [t[f"in.shifted_x.{k}"] for k in range(depth)], [t[f"in.shifted_y.{k}"] for k in range(depth)]


def test_restatement_reproduces_the_model_fixture_in_the_bf16_flow(fixture):
    """Same ops in the same dtype flow: logits and loss are within the rounding distance the fixture itself shows between its bf16 and fp32 flows."""
    t = fixture
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    cap = {}
    loss, logits = DO.model_loss(sd, CFG, *_inputs(t), capture=cap)
    own = DO.rel_l2(t["out.logits"], t["twin.logits"])
    assert logits.dtype == BF16 and DO.rel_l2(logits, t["out.logits"]) <= own, (DO.rel_l2(logits, t["out.logits"]), own)
    tol = abs(float(t["out.loss"]) - float(t["twin.loss"])) + 2.0 ** -7 * abs(float(t["twin.loss"]))  # plus one bf16 step of the loss
    assert abs(float(loss) - float(t["out.loss"])) <= tol
    for name in ("q", "k", "v", "ctx"):
        want = t["cap.block0." + name]
        assert cap[name].shape == want.shape and DO.rel_l2(cap[name], want) <= own, name
    assert (t["in.targets"] == -100).any() and (t["in.shifted_y.0"] == -100).any()


def test_restatement_matches_the_twin_in_the_fp32_flow(fixture):
    t = fixture
    sd32 = {k[3:]: (v.float() if v.is_floating_point() else v) for k, v in t.items() if k.startswith("sd.")}
    loss, logits = DO.model_loss(sd32, CFG, *_inputs(t))
    assert logits.dtype == torch.float32 and DO.rel_l2(logits, t["twin.logits"]) < 1e-5
    assert abs(float(loss) - float(t["twin.loss"])) / float(t["twin.loss"]) < 1e-5
    # and the fp64 flow on the bf16 weights (bf16-rounded tables) stays within the tables' rounding of the twin
    l64, _ = DO.model_loss({k[3:]: v for k, v in t.items() if k.startswith("sd.")}, CFG, *_inputs(t), dtype=torch.float64)
    assert abs(float(l64) - float(t["twin.loss"])) / float(t["twin.loss"]) < 1e-4


def test_restatement_gradients_match_the_twin(fixture):
    """autograd through the restatement in fp32 gives the twin's gradients: the restatement is the same function, not only the same value."""
    t = fixture
    sd32 = {k[3:]: (v.float() if v.is_floating_point() else v) for k, v in t.items() if k.startswith("sd.")}
    _, _, grads = DO.model_grads(sd32, CFG, *_inputs(t))
    seen = 0
    for k in t:
        if k.startswith("twin.grad.") and not DO.floor_allowed(k[10:]):
            assert DO.rel_l2(grads[k[10:]], t[k]) < 1e-4, k
            seen += 1
    assert seen >= 29
    for n, g in grads.items():  # the MTP block's output feeds nothing at mtp_depth = 1: no gradient in the reference, zero here
        if n.startswith("mtp_modules.0.trf_block."):
            assert "twin.grad." + n not in t and float(g.abs().max()) == 0.0


def test_restatement_reproduces_the_attention_fixture(mla_fixture):
    t = mla_fixture
    spec = DO.MLA_FIXTURE
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    cos, sin = DO.rope_tables(spec["rope_base"], spec["d_out"] // spec["num_heads"] // 2, spec["context_length"])
    y, dx, grads = DO.mla_grads(sd, t["in.x"], t["in.dy"], spec["num_heads"], cos, sin)
    assert y.dtype == BF16
    assert DO.rel_l2(y, t["out.y"]) <= DO.rel_l2(t["out.y"], t["twin.y"])
    assert DO.rel_l2(dx, t["out.dx"]) <= DO.rel_l2(t["out.dx"], t["twin.dx"])
    sd32 = {k: v.float() for k, v in sd.items()}
    y32, dx32, g32 = DO.mla_grads(sd32, t["in.x"].float(), t["in.dy"].float(), spec["num_heads"], cos, sin)
    assert DO.rel_l2(y32, t["twin.y"]) < 1e-5 and DO.rel_l2(dx32, t["twin.dx"]) < 1e-4
    for n in ("wk_decoup.weight", "wk_decoup.bias", "wkv_down_proj.weight", "wkv_down_proj.bias"):
        assert DO.rel_l2(g32[n], t["twin.grad." + n]) < 1e-4, n
        assert DO.rel_l2(t["out.grad." + n], t["twin.grad." + n]) <= 0.1, n


def test_signatures_and_state_dict_match_the_reference():
    A, B, M = _mods()
    sig = json.load(open(os.path.join(GOLDEN, "deepseek_signatures.json")))
    classes = dict(MultiLatentAttention=A.MultiLatentAttention, RMSNorm=B.RMSNorm, SiLU=B.SiLU, FFN=B.FFN, TransformerBlock=B.TransformerBlock,
                   MTPModule=M.MTPModule, MainModel=M.MainModel, DeepSeekV3Model=M.DeepSeekV3Model)
    assert set(sig["constructors"]) == set(classes)
    for name, cls in classes.items():
        assert [p for p in inspect.signature(cls.__init__).parameters if p != "self"] == sig["constructors"][name], name
    # forward signatures: the reference's names first, private extensions (leading underscore) only behind them
    fwd = lambda cls: [p for p in inspect.signature(cls.forward).parameters if p != "self" and not p.startswith("_")]
    for name, params in sig["forwards"].items():
        assert fwd(classes[name]) == params, name
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    m = M.DeepSeekV3Model(dict(CFG)).to(BF16)
    assert desc(m.state_dict()) == sig["state_dict"]
    assert m.mtp_modules[0].emb_layer is m.main_model.emb_layer and m.mtp_modules[0].out_layer is m.main_model.out_layer  # shared, as upstream
    spec = DO.MLA_FIXTURE
    att = A.MultiLatentAttention(spec["d_in"], spec["d_out"], spec["num_heads"]).to(BF16)
    assert desc(att.state_dict()) == sig["mla_state_dict"]
    assert att.q_rank == 1536 and att.kv_rank == 4 * att.head_dim and att.decoup_head_dim == att.head_dim // 2
    assert m.cos.shape == (CFG["context_length"], CFG["emb_dim"] // CFG["n_heads"] // 2)
    from llm_quest_amd import config

    c = config.DEEPSEEK_SMALL_CONFIG
    assert (c["emb_dim"], c["n_heads"], c["n_layers"], c["num_ffn"], c["mtp_depth"], c["mtp_loss_coeff"], c["vocab_size"]) == (768, 12, 12, 3, 2, 0.2, 50304)


def test_refusals():
    A, B, M = _mods()
    with pytest.raises(NotImplementedError, match="DeepSeekMoE"):
        B.TransformerBlock(dict(CFG), layer=CFG["num_ffn"])
    with pytest.raises(NotImplementedError, match="DeepSeekMoE"):
        M.DeepSeekV3Model(dict(CFG, n_layers=2))  # layer 1 >= num_ffn = 1
    with pytest.raises(ValueError, match="head_dim 32 not built"):
        A.MultiLatentAttention(64, 64, 2)
    m = M.DeepSeekV3Model(dict(CFG)).to(BF16)
    ids = torch.zeros(2, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(ids, ids, [ids], [ids])
    x = torch.zeros(2, 8, CFG["emb_dim"], dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.main_model.trf_blocks[0](x, m.mask, m.cos, m.sin)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.main_model.trf_blocks[0].att(x, m.mask, m.cos, m.sin)
    from llm_quest_amd import kernels_mla as KM
    from llm_quest_amd import ops_mla

    z = lambda w: torch.zeros(8, w, dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.mla_attn_fwd(z(64), z(32), z(64), z(32), z(64), 1, 8, 1, 64, 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.mla_rope_fwd(z(32), z(32), 8, 1, 32, torch.zeros(8, 32), torch.zeros(8, 32))
    with pytest.raises(TypeError, match=r"to\(torch.bfloat16\)"):
        ops_mla.check_bf16(M.DeepSeekV3Model(dict(CFG)), "DeepSeekV3Model")  # the norms and the MLA Linears are still fp32
    with pytest.raises(ValueError, match="causal mask"):
        ops_mla.check_mask(torch.zeros(8, 8, dtype=torch.bool), 8)
    ops_mla.check_mask(m.mask, 8)


def _entry_points():
    """(name, good arguments) of the four entry points on a 16-byte aligned host buffer: no kernel is ever launched by the calls below, each is
    refused by the validation first."""
    from llm_quest_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    B, S, H, Dn, Dr = 1, 8, 2, 64, 32
    fwd = [B, S, H, Dn, Dr, p, H * Dn, p, H * Dr, p, H * Dn, p, Dr, p, H * Dn, p, H * Dn, p, 0.1, None]
    bwd = [B, S, H, Dn, Dr, p, H * Dn, p, H * Dr, p, H * Dn, p, Dr, p, H * Dn, p, H * Dn, p, H * Dn, p, p, p, H * Dn, p, H * Dr, p, H * Dn, p, p, H * Dn, 0.1, None]
    rfwd = [B * S, S, H, Dr, p, H * Dr, p, Dr, p, p, S, p, H * Dr, p, Dr, None]
    rbwd = [B * S, S, H, Dr, p, H * Dr, p, p, p, S, p, H * Dr, p, Dr, None]
    return lib, buf, {"mi355_mla_attn_fwd": fwd, "mi355_mla_attn_bwd": bwd, "mi355_mla_rope_fwd": rfwd, "mi355_mla_rope_bwd": rbwd}


@pytest.mark.parametrize("name", ["mi355_mla_attn_fwd", "mi355_mla_attn_bwd", "mi355_mla_rope_fwd", "mi355_mla_rope_bwd"])
def test_entry_points_refuse_bad_calls_with_a_message(name):
    lib, _keep, calls = _entry_points()
    good = calls[name]
    attn = "attn" in name

    def refused(args, expect):
        rc = getattr(lib, name)(*args)
        msg = lib.mi355_last_error().decode()
        assert rc != 0 and msg and expect in msg, (name, rc, msg)

    bad = list(good)
    if attn:
        bad[3], bad[4] = 64, 64  # unsupported (Dn, Dr)
    else:
        bad[3] = 48
    refused(bad, "not built")
    bad = list(good)
    bad[5 if attn else 4] = None  # the first operand pointer
    refused(bad, "null pointer")
    bad = list(good)
    bad[1] = 0  # S = 0
    refused(bad, "must be")
    bad = list(good)
    bad[6 if attn else 5] = 8  # first leading dimension shorter than its row
    refused(bad, "leading dimension")


def test_fixture_floors_meet_the_condition(fixture):
    """The premise of the model test (tools/gen_golden_deepseek.py::check_floors): every gradient's bf16-vs-twin distance is <= 0.1 outside the
    named allow-list, whose members are far above it (true gradient zero), and at most 10 % of the gradient tensors lie outside."""
    t = fixture
    names = [k[10:] for k in t if k.startswith("twin.grad.")]
    assert len(names) == 30
    outside = 0
    for n in names:
        floor = DO.rel_l2(t["grad." + n], t["twin.grad." + n])
        if DO.floor_allowed(n):
            assert floor > 1e2, (n, floor)
        else:
            assert floor <= 0.1, (n, floor)
        outside += floor > 0.1
    assert outside * 10 <= len(names)
    sig = json.load(open(os.path.join(GOLDEN, "deepseek_signatures.json")))
    assert sig["perturbation_seed"] == 321 and set(sig["floors"]) == set(names)
