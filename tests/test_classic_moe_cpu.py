"""CPU-side checks of the classic-MoE path: constructor parameters, defaults and state_dict layout against the reference's
(tests/golden/classic_moe_signatures.json), ``hidden_dim``, the two assertions, every refusal by message, the new entry points in header and binding
table with their host-side validation (no launch), the fixture's own conditions, and the plain-torch restatement (tests/classic_moe_oracle.py) against
the fixture under the 1.5x rule (``test_deepseek_moe_gpu.judge``): that proves the yardstick the GPU tests use."""

import ctypes
import inspect
import json
import os
import re

import pytest
import torch

import classic_moe_oracle as CO
from test_deepseek_moe_gpu import judge

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi355_cmoe_route_fwd", "mi355_cmoe_route_bwd", "mi355_cmoe_loss", "mi355_cmoe_bias_act_fwd", "mi355_cmoe_segment_colsum")


def _sig():
    with open(os.path.join(CO.GOLDEN, "classic_moe_signatures.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fixture():
    return CO.load_fixture("classic_moe_tiny")


def _build(name, cls="MoE"):
    from llm_quest_amd.moe import classic_moe as M

    spec = CO.FIXTURE_LAYERS[name]
    return getattr(M, cls)(dict(spec["cfg"]), **spec["kwargs"]).to(BF16)


def test_signatures_defaults_and_state_dict_match_the_reference():
    from llm_quest_amd.moe import classic_moe as M

    sig = _sig()
    assert set(sig["constructors"]) == {"ExpertGeLU", "MoE", "MoE_old"}
    for name, order in sig["constructor_order"].items():
        params = {n: q for n, q in inspect.signature(getattr(M, name).__init__).parameters.items() if n != "self"}
        assert list(params) == order, name
        for n, q in params.items():
            want = sig["constructors"][name][n]
            assert (want == "<required>") if q.default is inspect.Parameter.empty else (q.default == want and type(q.default) is type(want)), (name, n, q.default, want)
    for cls in ("MoE", "MoE_old"):
        for name in CO.FIXTURE_LAYERS:
            sd, want = _build(name, cls).state_dict(), sig["state_dict"][name]
            assert list(sd) == list(_build(name).state_dict()) and set(sd) == set(want), (cls, name)
            for k, v in sd.items():
                assert list(v.shape) == want[k]["shape"] and str(v.dtype).replace("torch.", "") == want[k]["dtype"], (cls, name, k, v.shape, v.dtype, want[k])
    b = _build("B")
    assert (b.num_experts, b.top_k, b.load_coeff, b.z_router_coeff) == (8, 2, 10e-2, 1e-3) and b._forced_topk is None
    assert list(dict(b.experts[0].named_parameters())) == ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"]
    assert isinstance(b.experts[0].layers, torch.nn.Sequential) and len(b.experts[0].layers) == 3
    assert tuple(b.gate.weight.shape) == (8, 64) and tuple(b.gate.bias.shape) == (8,)
    assert issubclass(M.MoE_old, M.MoE)
    from llm_quest_amd import moe as pkg

    assert all(n in pkg.__doc__ for n in ("ExpertGeLU", "MoE", "MoE_old"))


def test_hidden_dim_for_auto_and_for_a_numeric_factor():
    from llm_quest_amd.moe.classic_moe import ExpertGeLU, MoE

    assert MoE(dict(emb_dim=64)).experts[0].hidden_dim == 128  # "auto": 4 * (1 / 2) * 64
    assert MoE(dict(emb_dim=64), num_experts=4, top_k=4).experts[0].hidden_dim == 64  # "auto": 1 / 4
    assert MoE(dict(emb_dim=80), num_experts=3, top_k=1, scaling_factor=0.125).experts[0].hidden_dim == 40
    assert MoE(dict(emb_dim=64), scaling_factor=1).experts[0].hidden_dim == 256
    ex = ExpertGeLU(dict(emb_dim=16), 0.5)
    assert ex.hidden_dim == 32 and tuple(ex.layers[0].weight.shape) == (32, 16) and tuple(ex.layers[2].weight.shape) == (16, 32)
    assert tuple(ex.layers[0].bias.shape) == (32,) and tuple(ex.layers[2].bias.shape) == (16,)


def test_the_two_assertions():
    from llm_quest_amd.moe.classic_moe import MoE, MoE_old

    for cls in (MoE, MoE_old):
        with pytest.raises(AssertionError, match="emb_dim must be divisible by scaling_factor"):
            cls(dict(emb_dim=64), scaling_factor=3)
        with pytest.raises(AssertionError, match="top_k must be > 0"):
            cls(dict(emb_dim=64), top_k=0)
        with pytest.raises(AssertionError, match="top_k must be > 0"):
            cls(dict(emb_dim=64), num_experts=2, top_k=3)


def test_refusals_fire_by_name():
    from llm_quest_amd.moe.classic_moe import ExpertGeLU, MoE

    assert MoE(dict(emb_dim=64), scaling_factor=0.0625).experts[0].hidden_dim == 16
    with pytest.raises(ValueError, match="hidden_dim.*multiple of 8"):
        MoE(dict(emb_dim=72), top_k=1, scaling_factor=0.125)  # int(4 * 0.125 * 72) = 36
    with pytest.raises(ValueError, match="hidden_dim.*multiple of 8"):
        ExpertGeLU(dict(emb_dim=24), 0.125)  # 12
    with pytest.raises(ValueError, match="emb_dim.*multiple of 8"):
        MoE(dict(emb_dim=60))
    with pytest.raises(ValueError, match="emb_dim.*multiple of 8"):
        ExpertGeLU(dict(emb_dim=12), 2)
    with pytest.raises(ValueError, match="num_experts must be at most 128"):
        MoE(dict(emb_dim=16), num_experts=129)
    with pytest.raises(ValueError, match="top_k must be at most 8"):
        MoE(dict(emb_dim=16), num_experts=16, top_k=9)
    assert MoE(dict(emb_dim=16), num_experts=128, top_k=8).num_experts == 128  # the limits themselves are in


def test_no_cpu_fallback_and_dtype_refusals():
    """``L.require_gpu`` speaks first on CPU tensors; the dtype refusals are the launch wrappers' own checks, called directly."""
    from llm_quest_amd import ops_cmoe
    from llm_quest_amd.moe.classic_moe import ExpertGeLU, MoE

    m, ex = MoE(dict(emb_dim=16), num_experts=2, top_k=1).to(BF16), ExpertGeLU(dict(emb_dim=16), 0.5).to(BF16)
    x = torch.zeros(1, 4, 16, dtype=BF16)
    for mod in (m, ex):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mod(x)
    with pytest.raises(TypeError, match="ExpertGeLU: parameter 'layers.0.weight' is torch.float32"):
        ops_cmoe.check_bf16(ExpertGeLU(dict(emb_dim=16), 0.5), "ExpertGeLU")
    with pytest.raises(TypeError, match="MoE: parameter 'experts.0.layers.0.weight' is torch.float32"):
        ops_cmoe.check_bf16(MoE(dict(emb_dim=16), num_experts=2), "MoE")
    ops_cmoe.check_bf16(m, "MoE")


def test_the_new_entry_points_are_declared_and_bound():
    from llm_quest_amd import _lib

    raw = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "llm_quest_amd", "csrc", "Makefile")).read(), flags=re.M).group(1).split()
    assert "classic_moe.hip" in srcs
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared in include/mi355_vlm.h"
        args = [a.strip() for a in m.group(1).split(",") if a.strip()]
        assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name]), name
        for a, t in zip(args, _lib.SIGNATURES[name]):
            want = ctypes.c_void_p if "*" in a else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_float if a.startswith("float") else ctypes.c_int
            assert t is want, (name, a, t)
        comment = raw[: raw.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "classic_moe.py:" in comment, f"{name}: the comment cites the reference lines it replaces"


def refusal_checks(lib, P=4096):
    """Refusal codes and messages of every new entry point.  Every call is refused on the host, before any launch: P is a non-null, 16-byte aligned
    address that is never dereferenced (the GPU test passes a dummy buffer's and checks that nothing was written)."""
    err = lambda: lib.mi355_last_error().decode()
    fwd, bwd, loss, act, seg = (getattr(lib, n) for n in ENTRY_POINTS)
    assert fwd(4, 0, 1, P, 8, None, P, 8, P, P, P, P, None) != 0 and "1..128" in err()
    assert fwd(4, 129, 1, P, 136, None, P, 136, P, P, P, P, None) != 0 and "1..128" in err()
    assert fwd(4, 7, 8, P, 8, None, P, 8, P, P, P, P, None) != 0 and "top_k" in err()
    assert fwd(4, 16, 9, P, 16, None, P, 16, P, P, P, P, None) != 0 and "top_k" in err()
    assert fwd(4, 16, 0, P, 16, None, P, 16, P, P, P, P, None) != 0 and "top_k" in err()
    assert fwd(4, 7, 3, None, 8, None, P, 8, P, P, P, P, None) != 0 and "null" in err()
    assert fwd(4, 7, 3, P, 8, None, P, 8, P, P, P, None, None) != 0 and "null" in err()  # lse
    assert fwd(4, 7, 3, P, 6, None, P, 8, P, P, P, P, None) != 0 and "leading dimension" in err()
    assert fwd(4, 7, 3, P, 8, None, P, 6, P, P, P, P, None) != 0 and "leading dimension" in err()
    assert fwd(1 << 31, 7, 3, P, 8, None, P, 8, P, P, P, P, None) != 0 and "2^31" in err()
    assert fwd(0, 0, 0, None, 0, None, None, 0, None, None, None, None, None) == 0  # an empty problem
    assert fwd(-3, 0, 0, None, 0, None, None, 0, None, None, None, None, None) == 0
    assert bwd(4, 0, 1, P, P, P, P, P, 8, None, None, 0.1, 1e-3, None, P, 8, None) != 0 and "1..128" in err()
    assert bwd(4, 7, 9, P, P, P, P, P, 8, None, None, 0.1, 1e-3, None, P, 8, None) != 0 and "top_k" in err()
    assert bwd(4, 7, 3, P, None, P, P, P, 8, None, None, 0.1, 1e-3, None, P, 8, None) != 0 and "null" in err()
    assert bwd(4, 7, 3, P, P, P, P, P, 8, None, P, 0.1, 1e-3, P, P, 8, None) != 0 and "counts" in err()  # g without the counts
    assert bwd(4, 7, 3, P, P, P, P, P, 8, P, P, 0.1, 1e-3, None, P, 8, None) != 0 and "logsumexp" in err()  # g without lse
    assert bwd(4, 7, 3, P, P, P, P, P, 8, None, None, 0.1, 1e-3, None, P, 6, None) != 0 and "leading dimension" in err()
    assert bwd(0, 0, 0, None, None, None, None, None, 0, None, None, 0.0, 0.0, None, None, 0, None) == 0
    assert loss(4, None, 1e-3, None, P, None) != 0 and "null" in err()
    assert loss(4, P, 1e-3, None, None, None) != 0 and "null" in err()
    assert loss(1 << 31, P, 1e-3, None, P, None) != 0 and "2^31" in err()
    assert loss(0, None, 0.0, None, None, None) == 0
    ok = (4, 16, 3, P, P, P, 16, P, 16, None, 0, P, 16, 1, None)  # R, N, E, counts, offsets, z, ldz, bias, stride_bias, pre, ldp, act, lda, kind

    def with_(i, v, args=ok):
        return args[:i] + (v,) + args[i + 1 :]

    assert act(*with_(13, 2)) != 0 and "kind" in err()
    assert act(*with_(2, 0)) != 0 and "1..128" in err()
    assert act(*with_(2, 129)) != 0 and "1..128" in err()
    assert act(*with_(1, 12)) != 0 and "multiple of 8" in err()
    assert act(*with_(1, 0)) != 0 and "multiple of 8" in err()
    assert act(*with_(0, 1 << 31)) != 0 and "2^31" in err()
    assert act(*with_(6, 8)) != 0 and "leading dimension" in err()
    assert act(*with_(6, 20)) != 0 and "leading dimension" in err()
    assert act(*with_(12, 8)) != 0 and "leading dimension" in err()  # act's pitch
    assert act(*with_(10, 8, with_(9, P))) != 0 and "leading dimension" in err()  # pre's pitch
    for i in (3, 4, 5, 7, 11):
        assert act(*with_(i, None)) != 0 and "null" in err(), i
    assert act(*with_(8, 12)) != 0 and "distance between two experts" in err()
    assert act(*with_(8, -8)) != 0 and "distance between two experts" in err()
    assert act(*with_(5, P + 2)) != 0 and "16-byte aligned" in err()
    assert act(*with_(7, P + 8)) != 0 and "16-byte aligned" in err()
    assert act(0, 0, 0, None, None, None, 0, None, 0, None, 0, None, 0, 0, None) == 0
    ok = (4, 16, 3, P, P, P, 16, P, 2, P, 16, 0, 0, None)  # R, N, E, counts, offsets, x, ldx, parts, n_parts, out, stride_out, out_dtype, accumulate
    assert seg(*with_(2, 0, ok)) != 0 and "1..128" in err()
    assert seg(*with_(2, 200, ok)) != 0 and "1..128" in err()
    assert seg(*with_(1, 20, ok)) != 0 and "multiple of 8" in err()
    assert seg(*with_(6, 8, ok)) != 0 and "leading dimension" in err()
    assert seg(*with_(8, 0, ok)) != 0 and "1..64" in err()
    assert seg(*with_(8, 65, ok)) != 0 and "1..64" in err()
    assert seg(*with_(11, 7, ok)) != 0 and "bf16 or fp32" in err()
    assert seg(*with_(10, 8, ok)) != 0 and "distance between two experts" in err()
    for i in (3, 4, 5, 7, 9):
        assert seg(*with_(i, None, ok)) != 0 and "null" in err(), i
    assert seg(*with_(5, P + 4, ok)) != 0 and "aligned" in err()
    assert seg(*with_(0, 1 << 31, ok)) != 0 and "2^31" in err()
    assert seg(0, 0, 0, None, None, None, 0, None, 0, None, 0, 0, 0, None) == 0


def test_host_side_validation_of_the_new_entry_points():
    """This machine has no GPU: whatever is refused here is refused before a launch."""
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    refusal_checks(_lib.load())


def test_the_launchers_refuse_on_the_host():
    from llm_quest_amd import kernels_cmoe as KC

    x = torch.zeros(4, 8, dtype=BF16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KC.route_fwd(x, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KC.loss(torch.zeros(4), 1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KC.bias_act_fwd(x, torch.zeros(1, 1, 8, dtype=BF16), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KC.segment_colsum(x, torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 1, 8))
    with pytest.raises(ValueError, match="contiguous bf16"):
        KC.gelu_bwd(torch.zeros(4, 16, dtype=BF16)[:, :8], x)


def test_fixture_meets_its_own_conditions(fixture):
    t, sig = fixture, _sig()
    for name, spec in CO.FIXTURE_LAYERS.items():
        pre = name + "."
        E, k, d = spec["E"], spec["k"], spec["cfg"]["emb_dim"]
        assert tuple(t[pre + "in.x"].shape) == (CO.FIXTURE_BATCH, CO.FIXTURE_SEQ, d) and t[pre + "in.x"].dtype == BF16
        p = torch.nn.functional.softmax(t[pre + "logits"], dim=-1)
        assert not bool(CO.boundary_tie(p, k).any()), "a boundary tie between the k-th and (k+1)-th probability"
        assert torch.equal(CO.topk_lowest_index_first(p, k)[1], t[pre + "topk_idxs"].long())
        assert isinstance(sig["seed"][name], int) and sig["seed"][name] >= 0
        floors = {n[len(pre + "twin.grad."):]: CO.rel_l2(t[pre + "grad." + n[len(pre + "twin.grad."):]], v) for n, v in t.items() if n.startswith(pre + "twin.grad.")}
        floors["out"], floors["moe_loss"] = CO.rel_l2(t[pre + "out"], t[pre + "twin.out"]), CO.rel_l2(t[pre + "moe_loss"], t[pre + "twin.moe_loss"])
        assert set(floors) == set(sig["floors"][name]) and max(floors.values()) <= 0.1, floors
        sd = {n[len(pre + "sd."):]: v for n, v in t.items() if n.startswith(pre + "sd.")}
        assert set(floors) == set(sd) | {"x", "out", "moe_loss"}, "every parameter has a gradient in the fixture"
        assert t[pre + "moe_loss"].dim() == 0 and t[pre + "moe_loss"].dtype == BF16 and all(v.dtype == BF16 for v in sd.values())
        assert all(float(v.float().abs().max()) > 0 for v in sd.values())
    assert CO.FIXTURE_LAYERS["A"]["hidden"] % 32 != 0 and CO.FIXTURE_LAYERS["A"]["E"] % 8 != 0


@pytest.mark.parametrize("name", list(CO.FIXTURE_LAYERS))
def test_the_restatement_reproduces_the_fixture(name, fixture):
    t, spec, pre = fixture, CO.FIXTURE_LAYERS[name], name + "."
    k, d = spec["k"], spec["cfg"]["emb_dim"]
    sd = {n[len(pre + "sd."):]: v for n, v in t.items() if n.startswith(pre + "sd.")}
    x, dy, g = t[pre + "in.x"].view(-1, d), t[pre + "in.dout"].view(-1, d), float(t[pre + "in.g"])
    rec = {}
    CO.layer(sd, x, k, record=rec)
    assert torch.equal(rec["logits"], t[pre + "logits"]) and torch.equal(rec["idx"], t[pre + "topk_idxs"].long()), "the reference flow's own selection"
    idx = t[pre + "topk_idxs"].long()
    out, loss, dx, grads, _ = CO.layer_grads(sd, x, k, dy, g, idx=idx)
    out64, loss64, dx64, grads64, _ = CO.layer_grads(sd, x, k, dy, g, dtype=F64, idx=idx)
    print(f"  bit-equal to the reference: out {torch.equal(out, t[pre + 'out'].view(-1, d))}, moe_loss {torch.equal(loss, t[pre + 'moe_loss'])}")
    bad = []
    rows = [("out", out, out64, t[pre + "out"], t[pre + "twin.out"]), ("moe_loss", loss, loss64, t[pre + "moe_loss"], t[pre + "twin.moe_loss"]),
            ("dx", dx, dx64, t[pre + "grad.x"], t[pre + "twin.grad.x"])]
    rows += [("d " + n, grads[n], grads64[n], t[pre + "grad." + n], t[pre + "twin.grad." + n]) for n in sd]
    for what, mine, mine64, ref, twin in rows:
        twin2 = twin.reshape(mine.shape)
        judge(what + " (reference flow)", mine, ref.reshape(mine.shape), twin2, bad)
        # the exact flow against the reference's own fp32 run: fp32's unit roundoff 6e-8 times the few thousand operations behind an element
        e = CO.rel_l2(mine64, twin2)
        if not e <= 1e-4:
            bad.append(f"{what}: the fp64 flow is {e:.3e} from the fp32 twin")
    assert not bad, "\n".join(bad)
