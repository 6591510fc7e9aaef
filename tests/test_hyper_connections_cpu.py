"""Hyper-connection Qwen3 without a GPU: the restatement (tests/hyper_oracle.py) against the reference fixture, and the drop-in surface
(state_dict layout, constructor parameters, what is refused) of llm_quest_amd.common.hyper_connections."""

import inspect
import json
import os

import pytest
import torch
import torch.nn as nn

import hyper_oracle as HO
from oracle.gen_golden import TINY_QWEN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 4


@pytest.fixture(scope="module")
def fixture():
    return HO.load_fixture()


@pytest.fixture(scope="module")
def signatures():
    with open(os.path.join(GOLDEN, "hyper_signatures.json")) as f:
        return json.load(f)


def test_restatement_reproduces_the_reference_fixture_bit_for_bit(fixture):
    t = fixture
    sd = {k[3:]: v for k, v in t.items() if k.startswith("sd.")}
    cap = {}
    with torch.no_grad():
        logits = HO.model(sd, TINY_QWEN, t["in.ids"], N, capture_block=1, capture=cap)
    assert logits.dtype == torch.bfloat16 and torch.equal(logits, t["out.logits"])
    for half in ("attn", "ffn"):
        for name in ("X", "R", "P", "Y", "Out"):
            assert torch.equal(cap[f"{half}.{name}"], t[f"cap.block1.{half}.{name}"]), f"{half}.{name}"
    from oracle import ops

    loss = ops.lm_loss(logits, t["in.targets"])
    assert loss.dtype == t["out.loss"].dtype and torch.equal(loss, t["out.loss"])


def test_fixture_floors_leave_every_gradient_judgeable_except_the_known_three(fixture):
    """The condition of the GPU model test, checked where the fixture is made too: the reference's own bf16-vs-fp32 gradient distance
    exceeds 0.1 at most for the three trf_blocks.0.hc_attn.pre.* tensors."""
    above = [k[len("twin.grad."):] for k in fixture if k.startswith("twin.grad.") and HO.rel_l2(fixture["grad." + k[len("twin.grad."):]], fixture[k]) > 0.1]
    assert all(n.startswith("trf_blocks.0.hc_attn.pre.") for n in above), above


def _tiny_model():
    from llm_quest_amd.common.hyper_connections.hyper_qwen3 import HyperQwen3Model

    return HyperQwen3Model(dict(TINY_QWEN), "hc", N).to(torch.bfloat16)


def test_state_dict_layout_and_initial_values_match_the_reference(signatures):
    m = _tiny_model()
    sd = m.state_dict()
    mine = {k: {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape)} for k, v in sd.items()}
    assert set(mine) == set(signatures["state_dict"])
    for k, ref in signatures["state_dict"].items():
        assert mine[k] == ref, (k, mine[k], ref)
    bf = lambda v: torch.tensor(v).to(torch.bfloat16).to(torch.float32)  # the cast to bf16 and back that model.to(bfloat16) puts the values through
    n_coeff = 0
    for i in range(TINY_QWEN["n_layers"]):
        for half in ("hc_attn", "hc_ffn"):
            pfx = f"trf_blocks.{i}.{half}."
            for conn, bias in (("res", torch.eye(N)), ("pre", torch.ones(N) / N), ("post", torch.ones(N))):
                for key in ("factor", "linear.weight", "bias"):
                    assert sd[pfx + f"{conn}.{key}"].dtype == torch.float32
                    n_coeff += 1
                assert torch.equal(sd[pfx + f"{conn}.factor"], bf([0.01]))
                assert torch.count_nonzero(sd[pfx + f"{conn}.linear.weight"]) == 0
                assert torch.equal(sd[pfx + f"{conn}.bias"], bf(bias.tolist()))
            assert sd[pfx + "norm.weight"].dtype == torch.bfloat16
    assert n_coeff == 18 * TINY_QWEN["n_layers"]


def test_fixture_state_dict_loads(fixture):
    m = _tiny_model()
    sd = {k[3:]: v for k, v in fixture.items() if k.startswith("sd.")}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and set(missing) <= {"mask", "cos", "sin", "out_head.weight"}, (missing, unexpected)
    assert m.trf_blocks[1].hc_ffn["res"].linear.weight.dtype == torch.float32


def test_constructor_parameter_names_match_the_reference(signatures):
    from llm_quest_amd.common.hyper_connections import hyper_connections as HC
    from llm_quest_amd.common.hyper_connections import hyper_qwen3 as HQ

    for cls in (HC.HyperConnectionRes, HC.HyperConnectionPre, HC.HyperConnectionPost, HQ.HyperQwen3TransformerBlock, HQ.HyperQwen3Model):
        mine = [p for p in inspect.signature(cls.__init__).parameters if p != "self"]
        assert mine == signatures["constructors"][cls.__name__], cls.__name__
    sig = inspect.signature(HC.HyperConnectionRes.__init__).parameters
    assert sig["expansion_rate"].default == 4 and sig["add_static_mapping"].default is True and sig["activation_cls"].default is nn.Tanh
    assert sig["device"].default is None and sig["h_dtypes"].default == torch.float32
    assert HC.HyperConnectionRes(16, 2, add_static_mapping=False).bias is None


@pytest.mark.parametrize("hc_type", ["mhc", "mhc-lite"])
def test_manifold_variants_are_refused_by_name(hc_type):
    from llm_quest_amd.common.hyper_connections.hyper_qwen3 import HyperQwen3Model, HyperQwen3TransformerBlock

    with pytest.raises(NotImplementedError, match=hc_type):
        HyperQwen3Model(dict(TINY_QWEN), hc_type, N)
    with pytest.raises(NotImplementedError, match="Sinkhorn"):
        HyperQwen3TransformerBlock(dict(TINY_QWEN), 0, hc_type, N)
    with pytest.raises(ValueError, match="Invalid Hyper-Connections type"):
        HyperQwen3Model(dict(TINY_QWEN), "nope", N)


def test_other_activations_dtypes_checkpointing_and_the_cache_are_refused():
    from llm_quest_amd.common.hyper_connections import hyper_connections as HC
    from llm_quest_amd.common.hyper_connections.hyper_qwen3 import HyperQwen3Model

    for cls in (HC.HyperConnectionRes, HC.HyperConnectionPre, HC.HyperConnectionPost):
        with pytest.raises(NotImplementedError, match="activation"):
            cls(128, 4, activation_cls=nn.Sigmoid)
        with pytest.raises(NotImplementedError, match="h_dtypes"):
            cls(128, 4, h_dtypes=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="gradient_checkpointing"):
        HyperQwen3Model(dict(TINY_QWEN, gradient_checkpointing=True), "hc", N)
    m = _tiny_model()
    m.gradient_checkpointing = True
    with pytest.raises(NotImplementedError, match="gradient_checkpointing"):
        m(torch.zeros(1, 4, dtype=torch.long))
    m.gradient_checkpointing = False
    with pytest.raises(NotImplementedError, match="KV-cache"):
        m(torch.zeros(1, 4, dtype=torch.long), kv_cache=object())


def test_no_cpu_fallback():
    from llm_quest_amd import kernels_hc as KH

    m = _tiny_model()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, dtype=torch.long))
    X, c, *_ = HO.make_operands(3, 4, 128, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.width_fwd(X, KH.Coeffs(*c))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KH.stream_sum(X)


def test_oracle_backward_flows_agree_with_each_other():
    """The two flows of the restatement are the two sides of the 1.5x rule: they must describe the same function (a mistake in one of them would
    move the yardstick).  Reference flow vs fp64 on a small problem, every output of the four arithmetic kernels."""
    X, c, Y, dOut, dP, dh_post = HO.make_operands(5, 4, 128, seed=3)
    R, P, H, TH = HO.width_fwd(X, c)
    Re, Pe, He, THe = HO.width_fwd(X, c, exact=True)
    for a, b in ((R, Re), (P, Pe), (H, He), (TH, THe)):
        assert HO.rel_l2(a, b) < 1e-2
    assert HO.rel_l2(HO.depth_fwd(Y, H[:, 5], R), HO.depth_fwd(Y, He[:, 5], Re, exact=True)) < 1e-2
    for a, b in zip(HO.depth_bwd(dOut, Y, H[:, 5]), HO.depth_bwd(dOut, Y, He[:, 5], exact=True)):
        assert HO.rel_l2(a, b) < 1e-2
    dX, g = HO.width_bwd(dOut, dP, dh_post, X, c)
    dXe, ge = HO.width_bwd(dOut, dP, dh_post, X, c, exact=True)
    assert HO.rel_l2(dX, dXe) < 1e-2
    assert set(g) == set(ge) == set(HO.Coeffs._fields)
    for k in g:
        assert HO.rel_l2(g[k], ge[k]) < 0.2, k  # sums over tokens with cancellation: a wrong formula is off by O(1), rounding by a few percent
