"""Qwen3 mixture-of-experts path without a GPU: the plain-torch restatement (tests/moe_oracle.py) against the reference fixture, signatures and
state_dict against the reference's, the new config entries, the refusals, the host-side validation of the entry points of csrc/moe.hip, and the
fixture's own conditions (no boundary tie, floors)."""

import ctypes
import inspect
import json
import os

import pytest
import torch

import moe_oracle as MO

BF16 = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CFG = MO.TINY_MOE


@pytest.fixture(scope="module")
def fixture():
    return MO.load_fixture()


def _sd(t, dtype=None):
    return {k[3:]: (v.to(dtype) if dtype is not None and v.is_floating_point() else v) for k, v in t.items() if k.startswith("sd.")}


def _probas(t, run="a."):
    return [t[f"{run}probas.{i}"] for i in range(CFG["n_layers"])]


def _lib():
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ----------------------------------------------------------------------------------------------------------------- restatement against the fixture
@pytest.mark.parametrize("run", ["a", "b"])
def test_restatement_reproduces_the_fixture_in_the_bf16_flow(fixture, run):
    """Same ops in the same dtype flow: logits, probabilities and loss are within the rounding distance the fixture itself shows between its
    bf16 and fp32 flows, and the selected experts are the reference's (the restatement's explicit top-k against the fixture's probabilities)."""
    t = fixture
    replay = _probas(t) if run == "b" else None
    loss, logits, ps = MO.model_loss(_sd(t), CFG, t["in.ids"], t["in.targets"], replay)
    own = MO.rel_l2(t[f"{run}.logits"], t[f"{run}.twin.logits"])
    assert logits.dtype == BF16 and MO.rel_l2(logits, t[f"{run}.logits"]) <= own, (MO.rel_l2(logits, t[f"{run}.logits"]), own)
    tol = abs(float(t[f"{run}.loss"]) - float(t[f"{run}.twin.loss"])) + 2.0 ** -7 * abs(float(t[f"{run}.twin.loss"]))  # plus one bf16 step of the loss
    assert abs(float(loss) - float(t[f"{run}.loss"])) <= tol
    for i, p in enumerate(ps):
        want = t[f"{run}.probas.{i}"]
        assert p.shape == want.shape == (MO.FIXTURE_BATCH * MO.FIXTURE_SEQ, CFG["num_experts"])
        assert MO.rel_l2(p, want) <= max(own, MO.rel_l2(want, t[f"{run}.twin.probas.{i}"])), i
        assert torch.equal(MO.topk_lowest_index_first(p, CFG["top_k"])[1], torch.topk(want, CFG["top_k"], dim=-1)[1]), i
    if run == "b":  # a replay returns the probabilities it was given
        assert all(torch.equal(t[f"b.probas.{i}"], t[f"a.probas.{i}"]) for i in range(CFG["n_layers"]))
    assert (t["in.targets"] == -100).any()


def test_restatement_matches_the_twin_in_the_fp32_and_fp64_flows(fixture):
    t = fixture
    for run, replay in (("a", None), ("b", _probas(t))):
        loss, logits, _ = MO.model_loss(_sd(t, torch.float32), CFG, t["in.ids"], t["in.targets"], replay)
        assert logits.dtype == torch.float32 and MO.rel_l2(logits, t[f"{run}.twin.logits"]) < 1e-5, run
        assert abs(float(loss) - float(t[f"{run}.twin.loss"])) / float(t[f"{run}.twin.loss"]) < 1e-5, run
    l64, logits64, _ = MO.model_loss(_sd(t), CFG, t["in.ids"], t["in.targets"], _probas(t), dtype=torch.float64)
    assert logits64.dtype == torch.float64 and abs(float(l64) - float(t["b.twin.loss"])) / float(t["b.twin.loss"]) < 1e-4


def test_restatement_gradients_match_the_twin(fixture):
    """autograd through the restatement in fp32 gives the twin's gradients of the replay run: the same function, not only the same value.  The
    gate has no gradient there, in the reference (None) and here (zero)."""
    t = fixture
    _, _, grads = MO.model_grads(_sd(t, torch.float32), CFG, t["in.ids"], t["in.targets"], _probas(t))
    seen = 0
    for k in t:
        if k.startswith("b.twin.grad."):
            assert MO.rel_l2(grads[k[12:]], t[k]) < 1e-4, k
            seen += 1
    assert seen == 67
    for n, g in grads.items():
        if n.endswith("moe.gate.weight"):
            assert "b.twin.grad." + n not in t and float(g.abs().max()) == 0.0


def test_fixture_conditions(fixture):
    """What tools/gen_golden_moe.py printed for the chosen seed, from the committed numbers: no boundary tie in either layer, every floor of the
    judged run at most 0.1 (FLOOR_ALLOW is empty)."""
    t = fixture
    sig = json.load(open(os.path.join(GOLDEN, "moe_signatures.json")))
    assert sig["boundary_ties"] == 0 and not MO.FLOOR_ALLOW
    for p in _probas(t):
        assert p.dtype == BF16 and not bool(MO.boundary_tie(p, CFG["top_k"]).any())
    floors = {k[12:]: MO.rel_l2(t["b.grad." + k[12:]], t[k]) for k in t if k.startswith("b.twin.grad.")}
    assert len(floors) == 67 and max(floors.values()) <= 0.1, max(floors.values())
    for name, f in floors.items():
        assert abs(f - sig["floors"][name]) <= 1e-3 * f + 1e-9, name


def test_plan_restatement_is_a_stable_sort():
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.randperm(8, generator=g)[:2] for _ in range(70)])
    counts, offsets, slot, row_token = MO.plan(idx, 8, 32)
    assert torch.equal(counts, torch.bincount(idx.flatten(), minlength=8)) and int(offsets[-1]) <= row_token.numel() == 70 * 2 + 8 * 31
    assert bool((offsets % 32 == 0).all()) and torch.equal(row_token[slot.flatten()], torch.arange(140) // 2)
    for e in range(8):
        rows = slot.flatten()[idx.flatten() == e]
        assert torch.equal(rows, torch.arange(int(offsets[e]), int(offsets[e]) + int(counts[e])))  # (t, j) ascending inside a segment
    assert int((row_token >= 0).sum()) == 140


# ----------------------------------------------------------------------------------------------------------------- interface
def _classes():
    from llm_quest_amd.moe import qwen3_moe as M
    from llm_quest_amd.qwen.qwen3 import qwen3_model as QM
    from llm_quest_amd.qwen.qwen3 import qwen3_transformer_block as QB

    return dict(Expert=M.Expert, Qwen3MoE=M.Qwen3MoE, MoETransformerBlock=QB.MoETransformerBlock, Qwen3MoEModel=QM.Qwen3MoEModel), M


def test_signatures_and_state_dict_match_the_reference():
    classes, M = _classes()
    sig = json.load(open(os.path.join(GOLDEN, "moe_signatures.json")))
    assert set(sig["constructors"]) == set(classes)
    for name, cls in classes.items():
        assert [p for p in inspect.signature(cls.__init__).parameters if p != "self"] == sig["constructors"][name], name
        # forward: the reference's names first, private extensions (leading underscore) only behind them
        assert [p for p in inspect.signature(cls.forward).parameters if p != "self" and not p.startswith("_")] == sig["forwards"][name], name
    assert list(inspect.signature(M.router_weights_init).parameters) == sig["functions"]["router_weights_init"]
    fwd = inspect.signature(classes["Qwen3MoEModel"].forward).parameters
    assert fwd["gate_probas"].default is None and fwd["return_gate_probas"].default is False and fwd["kv_cache"].default is None
    desc = lambda sd: {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    m = classes["Qwen3MoEModel"](dict(CFG)).to(BF16)
    assert desc(m.state_dict()) == sig["state_dict"]
    moe = m.trf_blocks[0].moe
    assert isinstance(moe.experts, torch.nn.ModuleList) and isinstance(moe.gate, torch.nn.Linear) and moe.gate.bias is None
    assert [n for n, _ in moe.experts[0].named_parameters()] == ["lin1.weight", "lin_gate.weight", "lin2.weight"]
    assert not hasattr(moe, "moe_loss")  # set by a training-mode forward only, as upstream
    assert len(m.arenas()) == CFG["n_layers"] + 1 and m.arenas()[0] is m.trf_blocks[-1]._arena  # backward-completion order


def test_router_weights_init_keeps_the_standard_deviation_and_equalises_the_row_norms():
    _, M = _classes()
    w = torch.randn(8, 64, generator=torch.Generator().manual_seed(3)) * torch.linspace(0.5, 4.0, 8).unsqueeze(1)
    std = float(w.std())
    M.router_weights_init(w)
    norms = torch.linalg.vector_norm(w, dim=-1)
    assert abs(float(w.std()) - std) < 1e-5 * std and float(norms.max() - norms.min()) < 1e-5 * float(norms.mean())


def test_new_config_entries():
    """The reference's dictionaries (config.py:289-318), written out."""
    from llm_quest_amd.config import qwen3_config_creator

    base = {"vocab_size": 151936, "rope_base": 1000000, "head_dim": 128, "dtype": torch.bfloat16, "model_type": "moe"}
    assert qwen3_config_creator("temp_moe") == dict(base, model_path="Qwen/Qwen3-temp_moe-Base", emb_dim=896, n_layers=12, n_heads=8, num_kv_groups=4,
                                                    moe_hidden_dim=3584, context_length=512, tie_embeddings=False, num_experts=16, top_k=4,
                                                    aux_loss_coef=0.001)
    assert qwen3_config_creator("30B-A3B", base_model=False) == dict(base, model_path="Qwen/Qwen3-30B-A3B", emb_dim=2048, n_layers=48, n_heads=32,
                                                                     num_kv_groups=4, hidden_dim=6144, moe_hidden_dim=768, context_length=40960,
                                                                     tie_embeddings=False, num_experts=128, top_k=8, aux_loss_coef=0.001)
    dense = qwen3_config_creator("0.6B")
    assert dense["model_type"] == "dense" and dense["hidden_dim"] == 3072 and "num_experts" not in dense
    with pytest.raises(KeyError):
        qwen3_config_creator("no such size")
    from llm_quest_amd.qwen.qwen3.qwen3_weight_loading import load_qwen3_weights

    with pytest.raises(NotImplementedError, match="MoE"):
        load_qwen3_weights(torch.nn.Linear(1, 1), qwen3_config_creator("temp_moe"), source={})


def test_refusals_fire_by_name():
    classes, M = _classes()
    with pytest.raises(NotImplementedError, match="shared_expert_hidden_dim"):
        M.Qwen3MoE(dict(CFG, shared_expert_hidden_dim=64))
    with pytest.raises(NotImplementedError, match="SiLU"):
        M.Expert(CFG, activation=torch.nn.functional.gelu)
    with pytest.raises(ValueError, match="top_k"):
        M.Qwen3MoE(dict(CFG, top_k=9, num_experts=8))  # k > E
    with pytest.raises(ValueError, match="num_experts"):
        M.Qwen3MoE(dict(CFG, num_experts=136))  # E > 128
    with pytest.raises(NotImplementedError, match="gradient_checkpointing"):
        classes["Qwen3MoEModel"](dict(CFG, gradient_checkpointing=True))
    m = classes["Qwen3MoEModel"](dict(CFG))
    ids = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="kv_cache"):
        m(ids, kv_cache=object())
    with pytest.raises(NotImplementedError, match="kv_cache"):
        m.trf_blocks[0](torch.zeros(1, 4, CFG["emb_dim"], dtype=BF16), m.mask, m.cos, m.sin, kv_cache=object())
    with pytest.raises(ValueError, match="gate_probas must be 2D"):
        m.trf_blocks[0].moe(torch.zeros(1, 4, CFG["emb_dim"], dtype=BF16), gate_probas=torch.zeros(1, 4, CFG["num_experts"]))
    with pytest.raises(ValueError, match="gate_probas must be 2D"):
        m.trf_blocks[0](torch.zeros(1, 4, CFG["emb_dim"], dtype=BF16), m.mask, m.cos, m.sin, gate_probas=torch.zeros(4))


def test_no_cpu_fallback():
    classes, M = _classes()
    from llm_quest_amd import kernels_moe as KM

    m = classes["Qwen3MoEModel"](dict(CFG))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, dtype=torch.long))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.trf_blocks[0].moe(torch.zeros(1, 4, CFG["emb_dim"], dtype=BF16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.route_fwd(torch.zeros(4, 8, dtype=BF16), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KM.plan(torch.zeros(4, 2, dtype=torch.int32), 8)


def test_entry_points_refuse_bad_calls_with_a_message():
    """Errors are returned (not faults): the ABI validates before launching.  The pointers are never dereferenced by a refused call."""
    lib = _lib()
    P = ctypes.c_void_p(4096)  # non-null, 16-byte aligned, never used
    err = lambda: lib.mi355_last_error()
    assert lib.mi355_moe_row_align() in (8, 16, 32, 64)
    assert lib.mi355_moe_plan_workspace_bytes(96, 8, 2) > 0 and lib.mi355_moe_plan_workspace_bytes(96, 200, 2) == 0
    # empty problems
    assert lib.mi355_moe_route_fwd(0, 8, 2, None, 8, 0, None, 8, None, None, None, None) == 0
    assert lib.mi355_moe_plan(-1, 8, 2, None, None, None, None, None, 0, None, 0.0, None, None, 0, None) == 0
    assert lib.mi355_moe_combine_fwd(0, 0, 2, 64, None, None, None, 64, None, 0, None, 64, None) == 0
    # limits
    assert lib.mi355_moe_route_fwd(4, 8, 9, P, 8, 0, P, 8, P, P, P, None) != 0 and b"top_k" in err()
    assert lib.mi355_moe_route_fwd(4, 4, 5, P, 8, 0, P, 8, P, P, P, None) != 0 and b"top_k" in err()  # k > E
    assert lib.mi355_moe_route_fwd(4, 129, 2, P, 136, 0, P, 136, P, P, P, None) != 0 and b"num_experts" in err()
    assert lib.mi355_moe_route_fwd(2 ** 30, 8, 8, P, 8, 0, P, 8, P, P, P, None) != 0 and b"2^31" in err()
    assert lib.mi355_moe_route_fwd(4, 8, 2, None, 8, 0, P, 8, P, P, P, None) != 0 and b"null" in err()
    assert lib.mi355_moe_route_fwd(4, 8, 2, P, 4, 0, P, 8, P, P, P, None) != 0 and b"leading dimension" in err()
    assert lib.mi355_moe_route_bwd(4, 8, 2, P, P, P, P, P, 8, None, P, 0.1, P, 8, None) != 0 and b"counts" in err()
    assert lib.mi355_moe_route_bwd(4, 8, 2, None, P, P, P, P, 8, None, None, 0.1, P, 8, None) != 0 and b"null" in err()
    align = lib.mi355_moe_row_align()
    need = 4 * 2 + 8 * (align - 1)
    assert lib.mi355_moe_plan(4, 8, 2, P, P, P, P, P, need - 1, None, 0.0, None, P, 1 << 20, None) != 0 and b"rows" in err()
    assert lib.mi355_moe_plan(4, 8, 2, P, P, P, P, P, need, None, 0.0, None, P, 0, None) != 0 and b"workspace" in err()
    assert lib.mi355_moe_plan(4, 8, 2, P, P, P, P, P, need, P, 0.0, None, P, 1 << 20, None) != 0 and b"load loss" in err()
    assert lib.mi355_moe_plan(4, 8, 2, None, P, P, P, P, need, None, 0.0, None, P, 1 << 20, None) != 0 and b"null" in err()
    # rows: width, pitches, alignment
    assert lib.mi355_moe_gather_rows(8, 4, 60, P, P, 64, P, 64, None) != 0 and b"multiple of 8" in err()
    assert lib.mi355_moe_gather_rows(8, 4, 64, P, P, 60, P, 64, None) != 0 and b"leading dimension" in err()
    assert lib.mi355_moe_gather_rows(8, 4, 64, P, ctypes.c_void_p(4098), 64, P, 64, None) != 0 and b"aligned" in err()
    assert lib.mi355_moe_gather_rows(8, 4, 64, None, P, 64, P, 64, None) != 0 and b"null" in err()
    assert lib.mi355_moe_combine_fwd(4, 8, 9, 64, P, P, P, 64, None, 0, P, 64, None) != 0 and b"top_k" in err()
    assert lib.mi355_moe_combine_fwd(4, 8, 2, 64, P, P, P, 64, P, 32, P, 64, None) != 0 and b"leading dimension" in err()
    assert lib.mi355_moe_combine_fwd(4, 8, 2, 64, P, None, None, 64, None, 0, P, 64, None) != 0 and b"null" in err()
    assert lib.mi355_moe_combine_bwd(4, 8, 2, 64, P, P, P, P, 64, None, 0, P, 64, P, None) != 0 and b"leading dimension" in err()  # dw without y
    assert lib.mi355_moe_combine_bwd(4, 8, 2, 64, P, P, None, P, 64, None, 0, None, 64, None, None) != 0 and b"null" in err()


def test_launchers_check_shapes_before_the_library_is_called():
    from llm_quest_amd import kernels_moe as KM

    with pytest.raises(ValueError, match="top_k"):
        KM.check_route(4, 4, 5)
    with pytest.raises(ValueError, match="num_experts"):
        KM.check_route(4, 129, 2)
    with pytest.raises(ValueError, match="2\\^31"):
        KM.check_route(2 ** 30, 8, 8)
    KM.check_route(130, 128, 8)
    # the combine's shared operand (DeepSeekMoE) needs the weights: refused on plain CPU tensors, before the device is asked for
    y, slot = torch.zeros(8, 64, dtype=BF16), torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="shared operand needs the weights"):
        KM.combine_fwd(y, slot, shared=torch.zeros(4, 64, dtype=BF16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # with the weights the call goes on to the device check
        KM.combine_fwd(y, slot, torch.zeros(4, 2, dtype=BF16), shared=torch.zeros(4, 64, dtype=BF16))
