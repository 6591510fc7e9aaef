"""CPU-side checks of the LatentMoE path: signatures and state_dict layout against the reference's (tests/golden/latent_moe_signatures.json), the
constructor's limits and ``cfg.get`` fallbacks, the new entry points in header and binding table, their host-side validation without a launch, the
fixture's own conditions, and the plain-torch restatement (tests/latent_moe_oracle.py) against the fixture."""

import ctypes
import inspect
import json
import os
import re

import pytest
import torch

import latent_moe_oracle as LO

BF16, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi355_latmoe_route_fwd", "mi355_latmoe_route_bwd", "mi355_latmoe_relu2_glu_fwd", "mi355_latmoe_relu2_glu_bwd")


def _sig():
    with open(os.path.join(LO.GOLDEN, "latent_moe_signatures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    return LO.load_fixture("latent_moe_tiny")


def _build(name):
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    spec = LO.FIXTURE_LAYERS[name]
    m = LatentMoE(dict(LO.FIXTURE_CFG), **spec["kwargs"])
    return m.to(BF16) if spec["to_bf16"] else m


def _cfg(**over):
    return dict(emb_dim=64, moe_hidden_dim=40, dtype=BF16, **over)


def test_signatures_and_state_dict_match_the_reference():
    from llm_quest_amd.moe import nvidia_latent_moe as M

    sig = _sig()
    assert set(sig["constructors"]) == {"SquaredReLU", "Expert", "LatentMoE"}
    for name, params in sig["constructors"].items():
        assert [p for p in inspect.signature(getattr(M, name).__init__).parameters if p != "self"] == params, name
    for name in LO.FIXTURE_LAYERS:
        sd, want = _build(name).state_dict(), sig["state_dict"][name]
        assert set(sd) == set(want), name
        for k, v in sd.items():
            assert list(v.shape) == want[k]["shape"] and str(v.dtype).replace("torch.", "") == want[k]["dtype"], (name, k, v.shape, v.dtype, want[k])
    a, b = _build("A"), _build("B")
    assert a.biases.dtype == F32 and b.biases.dtype == BF16  # plain construction / after .to(bfloat16): both must run
    assert "biases" in dict(a.named_buffers()) and "biases" not in dict(a.named_parameters())
    assert (a.num_experts, a.top_k, a.latent_dim) == (12, 4, 16) and (b.num_experts, b.top_k, b.latent_dim) == (16, 8, 16)
    assert tuple(a.gate.weight.shape) == (12, 64) and tuple(a.down_proj.weight.shape) == (16, 64) and tuple(a.up_proj.weight.shape) == (64, 16)
    assert a.shared_expert.hidden_dim == 48 and a.shared_expert.input_dim == 64
    assert all(ex.hidden_dim == 40 and ex.input_dim == 16 for ex in a.routed_experts)
    assert isinstance(a.shared_expert.activation, M.SquaredReLU) and a.routed_scaling_factor == 2.5 and a.bias_update_rate == 1e-3 and a._forced_topk is None


def test_routed_experts_are_built_with_moe_hidden_dim_as_upstream():
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    m = LatentMoE(_cfg(), routed_expert_hidden_dim=24, shared_expert_hidden_dim=56)
    assert m.routed_expert_hidden_dim == 24 and m.routed_experts[0].hidden_dim == 40  # stored, and not used: upstream's behaviour
    assert m.shared_expert_hidden_dim == 56 and m.shared_expert.hidden_dim == 56
    assert LatentMoE(_cfg()).shared_expert.hidden_dim == 40  # no shared size anywhere: moe_hidden_dim


def test_cfg_get_fallbacks():
    from llm_quest_amd.moe.nvidia_latent_moe import Expert, LatentMoE

    m = LatentMoE(_cfg())
    assert (m.top_k, m.num_experts) == (8, 16)  # 2 * 4 and 4 * 4
    m = LatentMoE(_cfg(), top_k=1, num_experts=3, latent_ratio=2)
    assert (m.top_k, m.num_experts, m.latent_dim) == (2, 6, 32)
    m = LatentMoE(_cfg(top_k=3, num_experts=5), top_k=1, num_experts=2)  # taken from cfg UNSCALED when present
    assert (m.top_k, m.num_experts) == (3, 5) and len(m.routed_experts) == 5 and tuple(m.biases.shape) == (5,)
    m = LatentMoE(_cfg(routed_scaling_factor=1.5, shared_expert_hidden_dim=24, routed_expert_hidden_dim=8), routed_scaling_factor=9.0, shared_expert_hidden_dim=72)
    assert m.routed_scaling_factor == 1.5 and m.shared_expert_hidden_dim == 24 and m.shared_expert.hidden_dim == 24 and m.routed_expert_hidden_dim == 8
    ex = Expert(_cfg())
    assert (ex.input_dim, ex.hidden_dim) == (64, 40) and list(dict(ex.named_parameters())) == ["lin1.weight", "lin_gate.weight", "lin2.weight"]
    ex = Expert(_cfg(), input_dim=16, hidden_dim=24)
    assert tuple(ex.lin1.weight.shape) == (24, 16) and tuple(ex.lin2.weight.shape) == (16, 24) and ex.lin1.weight.dtype == BF16


def test_constructor_limits():
    from llm_quest_amd.moe.nvidia_latent_moe import LatentMoE

    with pytest.raises(ValueError, match="divisible by latent_ratio"):
        LatentMoE(_cfg(), latent_ratio=3)
    with pytest.raises(ValueError, match="latent width.*multiple of 8"):
        LatentMoE(_cfg(), latent_ratio=16)  # 64 / 16 = 4
    with pytest.raises(ValueError, match="latent width.*multiple of 8"):
        LatentMoE(dict(_cfg(), emb_dim=48), latent_ratio=4)  # 12
    with pytest.raises(ValueError, match="moe_hidden_dim.*multiple of 8"):
        LatentMoE(dict(_cfg(), moe_hidden_dim=36))
    with pytest.raises(ValueError, match="moe_hidden_dim.*multiple of 8"):
        LatentMoE(dict(_cfg(), moe_hidden_dim=0))
    with pytest.raises(ValueError, match="shared expert's hidden size.*multiple of 8"):
        LatentMoE(_cfg(), shared_expert_hidden_dim=44)
    with pytest.raises(ValueError, match="shared expert's hidden size.*multiple of 8"):
        LatentMoE(_cfg(shared_expert_hidden_dim=-8))
    with pytest.raises(ValueError, match="1..128"):
        LatentMoE(_cfg(), top_k=1, num_experts=33)  # 132 experts
    with pytest.raises(ValueError, match="1..128"):
        LatentMoE(_cfg(num_experts=0))
    with pytest.raises(ValueError, match="top_k"):
        LatentMoE(_cfg(), top_k=3)  # 12 > 8
    with pytest.raises(ValueError, match="top_k"):
        LatentMoE(_cfg(top_k=0))
    with pytest.raises(ValueError, match="top_k"):
        LatentMoE(_cfg(top_k=5, num_experts=4))  # more than the experts
    for E in (1, 7, 128):  # any number of routed experts
        m = LatentMoE(_cfg(num_experts=E, top_k=1))
        assert m.num_experts == E and tuple(m.gate.weight.shape) == (E, 64)
    x = torch.zeros(1, 4, 64, dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LatentMoE(_cfg())(x)


def test_the_new_entry_points_are_declared_and_bound():
    from llm_quest_amd import _lib

    raw = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "llm_quest_amd", "csrc", "Makefile")).read(), flags=re.M).group(1).split()
    assert "latent_moe.hip" in srcs
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in include/mi355_vlm.h"
        args = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name]), name
        for a, t in zip(args, _lib.SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_float if a.startswith("float") else ctypes.c_int
            assert t is want, (name, a, t)
        comment = raw[: raw.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "nvidia_latent_moe.py:" in comment, f"{name}: the comment cites the reference lines it replaces"


def test_host_side_validation_of_the_new_entry_points():
    """Every refusal below returns an error code before any launch: this machine has no GPU."""
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused on the host
    err = lambda: lib.mi355_last_error().decode()
    fwd, bwd = lib.mi355_latmoe_route_fwd, lib.mi355_latmoe_route_bwd
    assert fwd(4, 0, 1, P, 8, P, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "1..128" in err()
    assert fwd(4, 129, 1, P, 136, P, 0, None, 2.5, P, 136, P, P, P, None) != 0 and "1..128" in err()
    assert fwd(4, 7, 8, P, 8, P, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "top_k" in err()
    assert fwd(4, 16, 9, P, 16, P, 0, None, 2.5, P, 16, P, P, P, None) != 0 and "top_k" in err()
    assert fwd(4, 7, 3, None, 8, P, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "null" in err()
    assert fwd(4, 7, 3, P, 8, None, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "biases" in err()
    assert fwd(4, 7, 3, P, 8, P, 5, None, 2.5, P, 8, P, P, P, None) != 0 and "bf16 or fp32" in err()
    assert fwd(4, 7, 3, P, 6, P, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "leading dimension" in err()
    assert fwd(1 << 31, 7, 3, P, 8, P, 0, None, 2.5, P, 8, P, P, P, None) != 0 and "2^31" in err()
    assert fwd(0, 0, 0, None, 0, None, 0, None, 0.0, None, 0, None, None, None, None) == 0  # an empty problem
    assert bwd(4, 0, 1, P, P, P, P, 8, 2.5, P, 8, None) != 0 and "1..128" in err()
    assert bwd(4, 7, 9, P, P, P, P, 8, 2.5, P, 8, None) != 0 and "top_k" in err()
    assert bwd(4, 7, 3, P, None, P, P, 8, 2.5, P, 8, None) != 0 and "null" in err()
    assert bwd(4, 7, 3, P, P, P, P, 8, 2.5, P, 6, None) != 0 and "leading dimension" in err()
    assert bwd(0, 0, 0, None, None, None, None, 0, 0.0, None, 0, None) == 0
    af, ab = lib.mi355_latmoe_relu2_glu_fwd, lib.mi355_latmoe_relu2_glu_bwd
    assert af(4, 12, P, 24, P, 16, None) != 0 and "multiple of 8" in err()
    assert af(4, 0, P, 16, P, 16, None) != 0 and "hidden size" in err()
    assert af(4, 16, P, 24, P, 16, None) != 0 and "leading dimension" in err()  # the pair's pitch is below 2F
    assert af(4, 16, P, 32, P, 8, None) != 0 and "leading dimension" in err()
    assert af(4, 16, P, 36, P, 16, None) != 0 and "leading dimension" in err()  # no multiple of 8
    assert af(4, 16, None, 32, P, 16, None) != 0 and "null" in err()
    assert af(4, 16, P + 2, 32, P, 16, None) != 0 and "16-byte" in err()
    assert af(1 << 31, 16, P, 32, P, 16, None) != 0 and "2^31" in err()
    assert af(0, 0, None, 0, None, 0, None) == 0
    assert ab(4, 12, P, 24, P, 16, P, 24, None) != 0 and "multiple of 8" in err()
    assert ab(4, 16, P, 32, P, 8, P, 32, None) != 0 and "leading dimension" in err()
    assert ab(4, 16, P, 32, P, 16, P, 24, None) != 0 and "leading dimension" in err()
    assert ab(4, 16, P, 32, P, 16, None, 32, None) != 0 and "null" in err()
    assert ab(4, 16, P, 32, P + 8, 16, P, 32, None) != 0 and "16-byte" in err()
    assert ab(0, 0, None, 0, None, 0, None, 0, None) == 0
    # the launchers refuse CPU tensors before anything else, and bad shapes before a pointer is taken
    from llm_quest_amd import kernels_latmoe as KL
    from llm_quest_amd import ops_moe
    from llm_quest_amd.moe.nvidia_latent_moe import Expert, SquaredReLU

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.route_fwd(torch.zeros(4, 7, dtype=BF16), torch.zeros(7, dtype=BF16), 3, 2.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.route_bwd(torch.zeros(4, 3), torch.ones(4), torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 7, dtype=BF16), 2.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.relu2_glu_fwd(torch.zeros(4, 32, dtype=BF16), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KL.relu2_glu_bwd(torch.zeros(4, 32, dtype=BF16), torch.zeros(4, 16, dtype=BF16), 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Expert(_cfg())(torch.zeros(1, 4, 64, dtype=BF16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SquaredReLU()(torch.zeros(4, 16, dtype=BF16))
    with pytest.raises(ValueError, match="'swiglu' or 'relu2'"):
        ops_moe._is_relu2("gelu")
    assert all(inspect.signature(f).parameters["activation"].default == "swiglu" for f in (
        ops_moe.run_experts_forward, ops_moe.run_experts_backward, ops_moe.experts_forward, ops_moe.experts_backward, ops_moe._experts_forward_loop,
        ops_moe._experts_backward_loop))


def test_the_fixture_meets_its_own_conditions(fixture):
    t, sig = fixture, _sig()
    for name, spec in LO.FIXTURE_LAYERS.items():
        E, k, pre = spec["E"], spec["k"], name + "."
        assert tuple(t[pre + "in.x"].shape) == (LO.FIXTURE_BATCH, LO.FIXTURE_SEQ, 64) and t[pre + "in.x"].dtype == BF16
        b0 = t[pre + "sd.biases"]
        assert b0.dtype == (BF16 if spec["to_bf16"] else F32) and bool((b0 != 0).any())
        if name == "A":
            assert torch.equal(b0, LO.bias_pattern(E)) and bool((b0.to(BF16).float() != b0).all())  # a pattern bf16 cannot hold
        logits = t[pre + "logits"]
        assert tuple(logits.shape) == (70, E) and not bool(LO.key_boundary_tie(logits, b0, k).any()), f"layer {name}: a boundary tie in the biased key"
        p = torch.sigmoid(logits)
        assert float(p.float().max()) < 1.0, "the sigmoid saturates"
        idx = t[pre + "topk_idxs"].long()
        mine = LO.topk_lowest_index_first(p + b0, k)[1]  # the same SET; inside it torch.topk orders equal keys as it likes, the restatement by index
        assert torch.equal(mine.sort(dim=1).values, idx.sort(dim=1).values)
        plain = LO.topk_lowest_index_first(p, k)[1]
        assert bool((plain.sort(dim=1).values != idx.sort(dim=1).values).any()), f"layer {name}: the biases change no selection"
        robust = t[pre + "robust"].bool()
        assert torch.equal(LO.robust_tokens(logits, b0, k), robust) and int(robust.sum()) * 10 >= 9 * robust.numel()
        assert torch.equal(LO.counts_of(idx, E), t[pre + "counts"].long())
        assert torch.equal(LO.bias_update(b0, t[pre + "counts"].long(), LO.RATE), t[pre + "biases"]) and not torch.equal(t[pre + "biases"], b0)
        names = [n[len(pre + "twin.grad."):] for n in t if n.startswith(pre + "twin.grad.")]
        assert set(names) == {n[len(pre + "grad."):] for n in t if n.startswith(pre + "grad.")} and "x" in names
        for n in names:
            floor = LO.rel_l2(t[pre + "grad." + n], t[pre + "twin.grad." + n])
            assert abs(floor - sig["floors"][name][n]) <= 1e-3 * floor + 1e-12, (name, n)
        assert all(os.path.getsize(os.path.join(LO.GOLDEN, f)) <= 1 << 20 for f in os.listdir(LO.GOLDEN) if f.startswith("latent_moe_"))


def test_the_restatement_reproduces_the_fixture(fixture):
    """The reference-flow layer of the restatement gives the reference's recorded output, logits, counts and updated biases EXACTLY, on its own
    selection and on the recorded one; its gradients are the reference's to within the order of the bf16 roundings in the backward."""
    t = fixture
    for name, spec in LO.FIXTURE_LAYERS.items():
        k, pre = spec["k"], name + "."
        sd = {n[len(pre + "sd."):]: v for n, v in t.items() if n.startswith(pre + "sd.")}
        x = t[pre + "in.x"].reshape(-1, 64)
        own, rec = {}, {}
        with torch.no_grad():
            LO.layer(sd, x, k, record=own)
            LO.layer(sd, x, k, idx=t[pre + "topk_idxs"].long(), record=rec)
        assert torch.equal(own["logits"], t[pre + "logits"])
        assert torch.equal(own["idx"].sort(dim=1).values, t[pre + "topk_idxs"].long().sort(dim=1).values)
        for r in (own, rec):
            assert torch.equal(r["out"], t[pre + "out"].reshape(-1, 64)), f"layer {name}: the restatement's output is not the reference's"
            assert torch.equal(r["counts"], t[pre + "counts"].long()) and torch.equal(r["biases"], t[pre + "biases"])
        dy = LO.loss_grad(t[pre + "out"].reshape(-1, 64))
        _, dx, grads, _ = LO.layer_grads(sd, x, k, dy, idx=t[pre + "topk_idxs"].long())
        _, dx64, grads64, _ = LO.layer_grads(sd, x, k, LO.loss_grad(t[pre + "twin.out"].reshape(-1, 64).double()), dtype=torch.float64, idx=t[pre + "topk_idxs"].long())
        assert LO.rel_l2(dx64, t[pre + "twin.grad.x"].reshape(-1, 64)) < 1e-5  # the fp64 flow is the fp32 twin to fp32 accuracy
        for n, g in grads.items():
            if pre + "grad." + n not in t:  # an expert without a token
                assert float(g.abs().max()) == 0.0, n
                continue
            floor = LO.rel_l2(t[pre + "grad." + n], t[pre + "twin.grad." + n])
            assert LO.rel_l2(g, t[pre + "twin.grad." + n]) <= 1.5 * floor + 2e-3, (name, n)
            assert LO.rel_l2(grads64[n], t[pre + "twin.grad." + n]) < 1e-4, (name, n)
