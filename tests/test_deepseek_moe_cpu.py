"""CPU-side checks of the DeepSeekMoE path: signatures and state_dict layout against the reference's (tests/golden/deepseek_moe_signatures.json),
the constructor's asserts and limits, the blocks that now construct, host-side validation of the new entry points without a launch, the fixture's
own conditions, and the plain-torch restatement (tests/deepseek_moe_oracle.py) against the fixture."""

import inspect
import json
import os

import pytest
import torch

import deepseek_moe_oracle as MO

BF16 = torch.bfloat16
CFG = MO.TINY_DEEPSEEK_MOE
LAYERS = MO.moe_layers(CFG)


def _sig():
    with open(os.path.join(MO.GOLDEN, "deepseek_moe_signatures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    return MO.load_fixture("deepseek_moe_tiny")


def _moe_cfg(**over):
    return dict(emb_dim=64, hidden_dim=128, dtype=BF16, num_experts=8, num_shared_experts=1, top_k=3, moe_scaling_factor="auto", moe_bias_update_rate=1e-3, **over)


def test_signatures_and_state_dict_match_the_reference():
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model
    from llm_quest_amd.moe import deepseek_moe as M

    sig = _sig()
    for name, params in sig["constructors"].items():
        assert [p for p in inspect.signature(getattr(M, name).__init__).parameters if p != "self"] == params, name
    for name, params in sig["functions"].items():
        assert list(inspect.signature(getattr(M, name)).parameters) == params, name
    m = DeepSeekV3Model(dict(CFG)).to(BF16)
    sd = m.state_dict()
    assert set(sd) == set(sig["state_dict"])
    for k, v in sd.items():
        want = sig["state_dict"][k]
        assert list(v.shape) == want["shape"] and str(v.dtype).replace("torch.", "") == want["dtype"], (k, v.shape, v.dtype, want)
    ffn = m.main_model.trf_blocks[LAYERS[0]].ffn
    assert isinstance(ffn, M.DeepSeekMoE) and tuple(ffn.shared_experts.lin1.weight.shape) == (1, 64, 32) and tuple(ffn.shared_experts.lin2.bias.shape) == (1, 64)
    assert "biases" in dict(ffn.named_buffers()) and "biases" not in dict(ffn.named_parameters()) and tuple(ffn.gate.weight.shape) == (7, 64)
    assert ffn.routed_experts[0].hidden_dim == 32  # "auto": 1 / (top_k + num_shared) of hidden_dim 128


def test_constructor_asserts_and_limits():
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    with pytest.raises(AssertionError, match="must be even"):
        DeepSeekMoE(dict(_moe_cfg(), top_k=2))  # 2 routed + 1 shared with "auto"
    with pytest.raises(AssertionError, match="must be even"):
        DeepSeekMoE(dict(_moe_cfg(), top_k=2, moe_scaling_factor=0.5))
    DeepSeekMoE(dict(_moe_cfg(), top_k=2, moe_scaling_factor=1))  # no parity condition at factor 1
    with pytest.raises(AssertionError, match="top_k must be > 0"):
        DeepSeekMoE(dict(_moe_cfg(), top_k=0, moe_scaling_factor=1))
    with pytest.raises(AssertionError, match="top_k must be > 0"):
        DeepSeekMoE(dict(_moe_cfg(), num_experts=3, num_shared_experts=1, top_k=3))
    with pytest.raises(ValueError, match="1..128"):
        DeepSeekMoE(dict(_moe_cfg(), num_experts=130, moe_scaling_factor=1))
    with pytest.raises(ValueError, match="top_k"):
        DeepSeekMoE(dict(_moe_cfg(), num_experts=16, num_shared_experts=0, top_k=10, moe_scaling_factor=1))
    with pytest.raises(ValueError, match="multiples of 8"):
        DeepSeekMoE(dict(_moe_cfg(), hidden_dim=36, moe_scaling_factor=1))
    with pytest.raises(ValueError, match="multiples of 8"):
        DeepSeekMoE(dict(_moe_cfg(), emb_dim=60, moe_scaling_factor=1))
    with pytest.raises(NotImplementedError, match="DeepSeekMoE.*num_experts"):
        DeepSeekMoE(dict(emb_dim=64, hidden_dim=128, dtype=BF16))
    for routed in (1, 7, 128):  # any number of routed experts
        moe = DeepSeekMoE(dict(_moe_cfg(), num_experts=routed, num_shared_experts=0, top_k=1, moe_scaling_factor=1, hidden_dim=8, emb_dim=8))
        assert moe.num_routed == routed and tuple(moe.biases.shape) == (routed,) and not hasattr(moe, "shared_experts")
    x = torch.zeros(1, 4, 64, dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeepSeekMoE(_moe_cfg()).to(BF16)(x)


def test_blocks_and_the_small_config_construct():
    from llm_quest_amd.config import DEEPSEEK_SMALL_CONFIG
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_model import DeepSeekV3Model
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_transformer_block import FFN, TransformerBlock
    from llm_quest_amd.moe.deepseek_moe import DeepSeekMoE

    cfg = dict(_moe_cfg(), n_heads=1, num_ffn=1)
    assert isinstance(TransformerBlock(cfg, layer=cfg["num_ffn"]).ffn, DeepSeekMoE)  # raised NotImplementedError before this layer existed
    assert isinstance(TransformerBlock(cfg, layer=0).ffn, FFN)
    with torch.device("meta"):
        m = DeepSeekV3Model(DEEPSEEK_SMALL_CONFIG)
    kinds = [type(b.ffn) for b in m.main_model.trf_blocks]
    assert kinds == [FFN] * 3 + [DeepSeekMoE] * 9
    assert all(isinstance(mod.trf_block.ffn, FFN) for mod in m.mtp_modules)
    moe = m.main_model.trf_blocks[3].ffn
    assert (moe.num_routed, moe.num_shared, moe.top_k, moe.routed_experts[0].hidden_dim) == (7, 1, 3, 768)


def test_arena_order_puts_lin_gate_in_front_of_lin1():
    from llm_quest_amd import ops_dsmoe
    from llm_quest_amd.llama3_to_deepseekv3.deepseek_transformer_block import TransformerBlock

    blk = TransformerBlock(dict(_moe_cfg(), n_heads=1, num_ffn=0), layer=0)
    names = [n for n, _ in ops_dsmoe.arena_named_params(blk)]
    assert sorted(names) == sorted(n for n, _ in blk.named_parameters())
    for e in range(7):
        i = names.index(f"ffn.routed_experts.{e}.lin_gate.weight")
        assert names[i + 1] == f"ffn.routed_experts.{e}.lin1.weight" and names[i + 2] == f"ffn.routed_experts.{e}.lin2.weight"
    assert list(blk.state_dict())[-1] == "ffn.gate.bias" and [n for n, _ in blk.named_parameters()].index("ffn.routed_experts.0.lin1.weight") < names.index(
        "ffn.routed_experts.0.lin1.weight")


def test_host_side_validation_of_the_new_entry_points():
    """Every refusal below returns an error code before any launch: this machine has no GPU."""
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
    err = lambda: lib.mi355_last_error().decode()
    assert lib.mi355_dsmoe_route_fwd(4, 0, 1, P, 8, P, 0, None, P, 8, P, P, P, None) != 0 and "1..128" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 129, 1, P, 136, P, 0, None, P, 136, P, P, P, None) != 0 and "1..128" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 8, P, 8, P, 0, None, P, 8, P, P, P, None) != 0 and "top_k" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 9, P, 8, P, 0, None, P, 8, P, P, P, None) != 0 and "top_k" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 3, None, 8, P, 0, None, P, 8, P, P, P, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 3, P, 8, None, 0, None, P, 8, P, P, P, None) != 0 and "biases" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 3, P, 8, P, 5, None, P, 8, P, P, P, None) != 0 and "bf16 or fp32" in err()
    assert lib.mi355_dsmoe_route_fwd(4, 7, 3, P, 6, P, 0, None, P, 8, P, P, P, None) != 0 and "leading dimension" in err()
    assert lib.mi355_dsmoe_route_fwd(1 << 31, 7, 3, P, 8, P, 0, None, P, 8, P, P, P, None) != 0 and "2^31" in err()
    assert lib.mi355_dsmoe_route_fwd(0, 0, 0, None, 0, None, 0, None, None, 0, None, None, None, None) == 0  # an empty problem
    assert lib.mi355_dsmoe_bias_update(0, P, P, 0, 1e-3, P, None) != 0 and "1..128" in err()
    assert lib.mi355_dsmoe_bias_update(129, P, P, 0, 1e-3, P, None) != 0 and "1..128" in err()
    assert lib.mi355_dsmoe_bias_update(7, None, P, 0, 1e-3, P, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_bias_update(7, P, P, 2, 1e-3, P, None) != 0 and "bf16 or fp32" in err()
    assert lib.mi355_dsmoe_bias_silu_fwd(4, 12, P, 16, P, P, 16, None) != 0 and "multiple of 8" in err()
    assert lib.mi355_dsmoe_bias_silu_fwd(4, 16, P, 8, P, P, 16, None) != 0 and "leading dimension" in err()
    assert lib.mi355_dsmoe_bias_silu_fwd(4, 16, P, 16, None, P, 16, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_bias_silu_fwd(4, 16, P + 2, 16, P, P, 16, None) != 0 and "16-byte" in err()
    assert lib.mi355_dsmoe_bias_silu_bwd(4, 0, P, 16, P, 16, P, 16, None) != 0 and "multiple of 8" in err()
    assert lib.mi355_dsmoe_bias_silu_bwd(4, 16, P, 16, P, 20, P, 16, None) != 0 and "leading dimension" in err()
    assert lib.mi355_dsmoe_bias_silu_bwd(4, 16, P, 16, P, 16, None, 16, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 100, 9, 64, P, P, P, 64, None, 0, None, 0, P, 64, None) != 0 and "top_k" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 100, 3, 60, P, P, P, 64, None, 0, None, 0, P, 64, None) != 0 and "multiple of 8" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 100, 3, 64, P, P, P, 64, P, 8, None, 0, P, 64, None) != 0 and "leading dimension" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 0, 3, 64, P, P, P, 64, None, 0, None, 0, P, 64, None) != 0 and "sorted rows" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 100, 3, 64, P, None, P, 64, None, 0, None, 0, P, 64, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_combine_fwd(4, 100, 3, 64, P, P, P, 64, None, 0, P + 8, 64, P, 64, None) != 0 and "16-byte" in err()
    assert lib.mi355_dsmoe_colsum_parts(0, 16, P, 16, P, 4, None) != 0 and "no rows" in err()
    assert lib.mi355_dsmoe_colsum_parts(4, 12, P, 16, P, 4, None) != 0 and "multiple of 8" in err()
    assert lib.mi355_dsmoe_colsum_parts(4, 16, P, 16, P, 0, None) != 0 and "row parts" in err()
    assert lib.mi355_dsmoe_colsum_parts(4, 16, P, 16, P, 2000, None) != 0 and "row parts" in err()
    assert lib.mi355_dsmoe_colsum_parts(4, 16, None, 16, P, 4, None) != 0 and "null" in err()
    assert lib.mi355_dsmoe_colsum_parts(4, 16, P + 4, 16, P, 4, None) != 0 and "16-byte" in err()
    # the launchers refuse CPU tensors before anything else
    from llm_quest_amd import kernels_dsmoe as KD

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.route_fwd(torch.zeros(4, 7, dtype=BF16), torch.zeros(7, dtype=BF16), 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.bias_update(torch.zeros(7, dtype=torch.int32), torch.zeros(7, dtype=BF16), 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.bias_silu_fwd(torch.zeros(4, 16, dtype=BF16), torch.zeros(16, dtype=BF16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KD.colsum(torch.zeros(4, 16, dtype=BF16))


def test_the_fixture_meets_its_own_conditions(fixture):
    t, k = fixture, CFG["top_k"]
    sig = _sig()
    assert float(t["in.targets"].eq(-100).sum()) > 0 and tuple(t["in.ids"].shape) == (MO.FIXTURE_BATCH, MO.FIXTURE_SEQ)
    for i in LAYERS:
        pre = f"moe.{i}."
        b0 = t[f"sd.main_model.trf_blocks.{i}.ffn.biases"]
        assert b0.dtype == BF16 and bool((b0 != 0).any())
        logits = t[pre + "logits"]
        assert not bool(MO.key_boundary_tie(logits, b0, k).any()), f"layer {i}: a boundary tie in the biased key"
        p = torch.nn.functional.softmax(logits, dim=-1)
        idx = t[pre + "topk_idxs"].long()
        mine = MO.topk_lowest_index_first(p + b0, k)[1]  # the same SET; inside it torch.topk orders equal keys as it likes, the restatement by index
        assert torch.equal(mine.sort(dim=1).values, idx.sort(dim=1).values)
        keys = (p + b0).gather(1, idx)
        assert bool((keys[:, 1:] <= keys[:, :-1]).all()) and bool(((mine == idx) | (keys == (p + b0).gather(1, mine))).all())
        plain = MO.topk_lowest_index_first(p, k)[1]
        assert bool((plain.sort(dim=1).values != idx.sort(dim=1).values).any()), f"layer {i}: the biases change no selection"
        assert torch.equal(MO.robust_tokens(logits, b0, k), t[pre + "robust"].bool())
        assert torch.equal(MO.counts_of(idx, 7), t[pre + "counts"].long())
    first = t[f"moe.{LAYERS[0]}.robust"]
    assert int(first.sum()) * 10 >= 9 * first.numel()
    outside, total = 0, 0
    for name in (n[len("twin.grad."):] for n in t if n.startswith("twin.grad.")):
        floor = MO.rel_l2(t["grad." + name], t["twin.grad." + name])
        assert abs(floor - sig["floors"][name]) <= 1e-3 * floor + 1e-12, name
        total += 1
        if floor > 0.1:
            outside += 1
            assert MO.floor_allowed(name), (name, floor)
    assert total == len(sig["floors"]) and outside * 10 <= total


def _judge(name, mine, ref_flow, exact):
    floor, got = MO.rel_l2(ref_flow, exact), MO.rel_l2(mine, exact)
    bound = 1.5 * floor + (0.0 if floor >= 1e-2 else 2e-3)
    print(f"  {name}: restatement {got:.3e}  reference {floor:.3e}  bound {bound:.3e}")
    assert got <= bound, (name, got, bound)


def test_the_restatement_reproduces_the_fixture(fixture):
    t = fixture
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    for i in LAYERS:
        pre, pfx = f"moe.{i}.", f"main_model.trf_blocks.{i}.ffn."
        rec, rec64 = {}, {}
        own = {}
        MO.moe_layer(sd, pfx, t[pre + "x"], CFG, record=own)  # its own selection: the reference's set (the order among equal keys is torch.topk's)
        assert torch.equal(own["logits"], t[pre + "logits"])
        assert torch.equal(own["idx"].sort(dim=1).values, t[pre + "topk_idxs"].long().sort(dim=1).values)
        MO.moe_layer(sd, pfx, t[pre + "x"], CFG, idx=t[pre + "topk_idxs"].long(), record=rec)
        assert torch.equal(rec["counts"], t[pre + "counts"].long()) and torch.equal(own["counts"], rec["counts"])
        assert torch.equal(rec["biases"], t[pre + "biases"])
        MO.moe_layer(sd, pfx, t[pre + "x"], CFG, dtype=torch.float64, idx=rec["idx"], record=rec64)
        _judge(pre + "out", rec["out"], t[pre + "out"], rec64["out"])
        _judge(pre + "max_vio", rec["max_vio"].reshape(1), t[pre + "max_vio"], rec64["max_vio"].reshape(1))
    # the model: loss and logits of the restatement's reference flow (its own selection per layer) against the fixture and the twin
    ids, y = t["in.ids"], t["in.targets"]
    sx, sy = [t["in.shifted_x.0"]], [t["in.shifted_y.0"]]
    idxs = {i: t[f"moe.{i}.topk_idxs"].long() for i in LAYERS}
    with torch.no_grad():
        loss, logits = MO.model_loss(sd, CFG, ids, y, sx, sy, idxs=idxs)
    _judge("logits", logits, t["out.logits"], t["twin.logits"])
    _judge("loss", loss.reshape(1), t["out.loss"].reshape(1), t["twin.loss"].reshape(1))
