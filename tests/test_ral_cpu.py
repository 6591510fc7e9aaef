"""Reinforced Attention Learning without a GPU: the signatures against the reference's, the plain-torch restatement (tests/ral_oracle.py) against
the reference fixture, the structural facts the kernels rely on (entries that hold exactly 1e-8 and add exactly 0), the refusals, the host-side
validation of the new entry points, and the fp32 emulation of the kernels' rounding points under the judgement of the GPU sweep."""

import inspect
import json
import os

import pytest
import torch

import ral_oracle as RO

GOLDEN = RO.GOLDEN
RTOL = 1e-5  # two orders above the reference's own fp32-vs-fp64 gap (tools/gen_golden_ral.py prints it)


@pytest.fixture(scope="module")
def gold():
    return RO.load_golden()


@pytest.fixture(scope="module")
def sig():
    return json.load(open(os.path.join(GOLDEN, "ral_signatures.json")))


def _mod():
    from llm_quest_amd.common import reinforced_attention_learning as R

    return R


def test_signatures_match_the_reference(sig):
    R = _mod()
    params = lambda fn: [[n, None if p.default is inspect.Parameter.empty else p.default] for n, p in inspect.signature(fn).parameters.items() if n != "self"]
    C = R.AttentionDivergenceLoss
    for name, want in sig["AttentionDivergenceLoss"].items():
        assert params(getattr(C, name)) == want, name
    assert params(R.attention_divergence_loss) == sig["attention_divergence_loss"]
    for name in sig["static_methods"]:
        assert isinstance(inspect.getattr_static(C, name), staticmethod), name
    m = C()
    assert m.ral_factor == 1.0 and m.diag_mask is None and m.q_norm_attn_weights is None and m.qlog_q is None
    assert [n for n in inspect.signature(R.prepare_attention_weights_from_qk).parameters] == [
        "q", "k", "b", "s", "num_heads", "num_kv_groups", "head_dim", "key_mask", "scale"]
    assert callable(R.collect_exposed_qk)


def test_forward_before_precompute_raises_the_reference_error(sig):
    R = _mod()
    with pytest.raises(RuntimeError) as e:
        R.AttentionDivergenceLoss()(torch.zeros(1, 1, 2, 2), torch.zeros(1), torch.zeros(1, 2))
    assert str(e.value) == sig["forward_before_precompute"]


def test_cpu_tensors_are_refused():
    R = _mod()
    w = torch.softmax(torch.randn(1, 2, 4, 4), dim=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.attention_divergence_loss(w, w, torch.zeros(1), torch.ones(1, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.AttentionDivergenceLoss().precompute_q_and_mask(w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.AttentionDivergenceLoss._prepare_attention_weights(w, torch.eye(4, dtype=torch.bool))
    q = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.prepare_attention_weights_from_qk(q, q[:, :64], 1, 4, 2, 1, 64)


def test_expose_qk_defaults_to_false():
    from llm_quest_amd.gpt_to_llama3.llama_attention import GroupedQueryAttention

    att = GroupedQueryAttention(128, 128, 2, 1, dtype=torch.bfloat16)
    assert att.expose_qk is False and att.exposed_qk is None
    R = _mod()

    class M:
        trf_blocks = [type("B", (), {"att": att})()]

    with pytest.raises(RuntimeError, match="expose_qk"):
        R.collect_exposed_qk(M())


@pytest.mark.parametrize("case", ["inline", "causal33", "causal65", "dense48"])
def test_restatement_reproduces_the_reference(gold, case):
    """Loss and gradient with respect to the policy weights, both entry points of the reference, and the prepared distribution."""
    g = lambda n: gold[f"{case}.{n}"]
    factor = float(g("ral_factor"))
    w = g("policy").clone().requires_grad_(True)
    loss = RO.ral_loss_from_weights(w, g("old"), g("adv"), g("loss_mask"), factor)
    (grad,) = torch.autograd.grad(loss, w)
    torch.testing.assert_close(RO.prepare_from_weights(g("policy"))[0], g("P"), rtol=RTOL, atol=0)
    for form in ("fn", "cls"):  # the class and function forms agree
        torch.testing.assert_close(loss.reshape(1), g("loss_" + form), rtol=RTOL, atol=1e-9)
        assert RO.rel_l2(grad, g("grad_" + form)) <= RTOL, form
    # the kernels' explicit backward formulas are the same gradient
    P, Z, _ = RO.prepare_from_weights(g("policy"))
    rows = RO.emulate_rows(P, Z, RO.prepare_from_weights(g("old"))[0], g("adv"), g("loss_mask"), factor, causal=False)
    assert RO.rel_l2(rows["da"].unsqueeze(1).expand_as(w) / w.shape[1], g("grad_fn")) <= RTOL
    torch.testing.assert_close(rows["loss"].reshape(1), g("loss_fn"), rtol=RTOL, atol=1e-9)


def test_masked_diagonal_and_upper_entries_hold_the_clamp_and_add_nothing():
    """Masked, diagonal and upper entries of P are exactly 1e-8 (as fp32 holds it) and contribute exactly 0 to the JSD, in every flow."""
    c = (2, 33, 4, 2, 64, "left", 1.0)
    ops = RO.operands(c, 5)
    B, S = 2, 33
    dead = ~RO.visible(B, S, ops["key_mask"])[:, 0] | torch.eye(S, dtype=torch.bool)
    for dtype in (RO.F32, RO.F64):
        P = RO.prepare_from_qk(ops["q"], ops["k"], ops["key_mask"], dtype=dtype)[0]
        Q = RO.prepare_from_qk(ops["q_old"], ops["k_old"], ops["key_mask"], dtype=dtype)[0]
        assert bool((P[dead] == RO.EPS).all()) and bool((Q[dead] == RO.EPS).all())
        M = (P + Q) / 2
        term = P * torch.log(P / M) + Q * torch.log(Q / M)
        assert bool((term[dead] == 0).all())
    Pe = RO.emulate_qk_fwd(ops["q"], ops["k"], ops["key_mask"])[0]
    assert bool((Pe[dead] == RO.EPS).all())
    assert RO.EPS == float(torch.tensor(1e-8, dtype=torch.float32))
    # rows with no visible key below the diagonal: row 0, the first real token behind the left padding, the padded rows themselves
    first = int(ops["key_mask"][0].argmax())
    for i in (0, first, first - 1):
        assert bool((Pe[0, i] == RO.EPS).all())


def test_host_side_validation_of_the_entry_points():
    from llm_quest_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    err = lambda: lib.mi355_last_error().decode()
    assert lib.mi355_ral_qk_prepare_fwd(1, 4, 4, 2, 96, None, 0, None, 0, None, 1.0, None, None, None, None) != 0 and "head_dim" in err()
    assert lib.mi355_ral_qk_prepare_fwd(1, 4, 3, 2, 64, None, 192, None, 128, None, 1.0, None, None, None, None) != 0 and "multiple" in err()
    assert lib.mi355_ral_qk_prepare_fwd(1, 4, 4, 2, 64, None, 256, None, 128, None, 1.0, None, None, None, None) != 0 and "null" in err()
    assert lib.mi355_ral_qk_prepare_fwd(0, 4, 4, 2, 64, None, 256, None, 128, None, 1.0, None, None, None, None) == 0
    assert lib.mi355_ral_qk_prepare_bwd(1, 4, 4, 2, 64, None, 256, None, 128, None, 1.0, None, None, None, None, 250, None, 128, None) != 0
    assert lib.mi355_ral_prepare_fwd(1, 0, 4, None, 1, None, None, None) != 0 and "head count" in err()
    assert lib.mi355_ral_prepare_fwd(1, 2, 4, None, 7, None, None, None) != 0 and "dtype" in err()
    assert lib.mi355_ral_prepare_bwd(1, 2, 4, None, None, 1, None) != 0 and "null" in err()
    assert lib.mi355_ral_renorm_bwd(1, 4, None, None, None, 2, None, None) != 0 and "causal" in err()
    assert lib.mi355_ral_jsd_fwd(1, 4, None, None, None, None) != 0 and "null" in err()
    assert lib.mi355_ral_jsd_bwd(-1, 4, None, None, None, None, None) != 0
    assert lib.mi355_ral_reduce(0, 4, None, None, None, 1.0, None, None, None, None) != 0 and "bad batch" in err()
    assert lib.mi355_ral_add_bf16(4, None, None, None, None) != 0 and "null" in err()
    assert lib.mi355_ral_add_bf16(0, None, None, None, None) == 0


def test_launchers_check_shapes_before_a_pointer_leaves():
    """The checks that do not need a device run first in the order device -> shape; on a CPU tensor the device check answers."""
    from llm_quest_amd import kernels_ral as KR

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KR.jsd_fwd(torch.zeros(1, 2, 2), torch.zeros(1, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KR.reduce(torch.zeros(1, 2), torch.zeros(1), torch.zeros(1, 2))


_emulated = {}


@pytest.mark.parametrize("c", RO.sweep_cases(), ids=RO.case_id)
def test_emulation_passes_the_judgement(c):
    """The fp32 emulation of the kernels' rounding points under the judgement of the GPU sweep; prints what the caps of the fp32 tensors come from."""
    B, S, Hq, Hkv, D, mask, qs = c
    ops = RO.operands(c, 1000 + S)
    exact, floor = RO.chain(ops, RO.F64), RO.chain(ops, RO.F32)
    assert float((exact["dP"] - exact["dP_autograd"]).abs().max()) <= 1e-12 * max(1.0, float(exact["dP"].abs().max()))
    got = RO.emulate_chain(ops)
    got["dq"], got["dk"] = RO.emulate_qk_bwd(ops["q"], ops["k"], got.pop("p"), exact["da"].float())
    worst, rels, fails = RO.judge_case(got, exact, floor)
    _emulated[RO.case_id(c)] = (worst, rels)
    print(f"[ral emulation] {RO.case_id(c)}: ratio " + " ".join(f"{n} {w:.3f}" for n, w in worst.items()) + " | rel " + " ".join(f"{n} {r:.2e}" for n, r in rels.items()))
    assert not fails, "\n".join(fails[:8])


@pytest.mark.parametrize("case", ["inline", "causal33", "causal65", "dense48"])
def test_emulation_of_the_materialised_path(gold, case):
    """The row kernels' formulas in fp32 on the reference's inputs under the judgement the GPU test applies: P, loss and dweights."""
    g = lambda n: gold[f"{case}.{n}"]
    factor = float(g("ral_factor"))
    w64 = g("policy").double().requires_grad_(True)
    loss64 = RO.ral_loss_from_weights(w64, g("old").double(), g("adv").double(), g("loss_mask"), factor)
    (grad64,) = torch.autograd.grad(loss64, w64)
    loss64 = loss64.detach()
    P, Z, _ = RO.prepare_from_weights(g("policy"))
    rows = RO.emulate_rows(P, Z, RO.prepare_from_weights(g("old"))[0], g("adv"), g("loss_mask"), factor, causal=False)
    B, H, S, _ = g("policy").shape
    P64, Z64, a64 = RO.prepare_from_weights(g("policy"), RO.F64)
    excl = RO.near_clamp(a64, Z64)
    assert float(excl.sum()) / excl.numel() <= RO.MAX_EXCLUDED_SHARE
    rows_of = lambda x: x.transpose(1, 2).reshape(B, 1, S, H * S)
    dw = (rows["da"] / H).unsqueeze(1).expand(B, H, S, S)
    wd, rd, fails = RO.judge_blocks("dweights", rows_of(dw), rows_of(grad64), rows_of(g("grad_fn")), RO.FP32_CAP["dweights"],
                                    excl[:, :, None, :].expand(B, S, H, S).reshape(B, 1, S, H * S))
    wp, rp, fp = RO.judge_blocks("P", P, P64, g("P"), RO.FP32_CAP["P"])
    rl = abs(float(rows["loss"]) - float(loss64)) / abs(float(loss64))
    print(f"[ral emulation] {case}: block rel l2 P {rp:.2e} dweights {rd:.2e} loss {rl:.2e}")
    assert not fails + fp, "\n".join((fails + fp)[:8])
    assert rl <= max(1.5 * abs(float(g("loss_fn")) - float(loss64)) / abs(float(loss64)), RO.FP32_CAP["loss"])


def test_emulation_summary_and_the_scaled_construction():
    """Runs after the table: the CPU column of ral_oracle.MEASURED; and the scaled operands do what the table wants of them."""
    if len(_emulated) == len(RO.sweep_cases()):
        names = sorted({n for w, _ in _emulated.values() for n in w})
        print("[ral emulation] worst ratio: " + "  ".join(f"{n} {max(w.get(n, 0) for w, _ in _emulated.values()):.3f}" for n in names))
        print("[ral emulation] worst block rel l2: " + "  ".join(f"{n} {max(r.get(n, 0) for _, r in _emulated.values()):.2e}" for n in names if n != "lse"))
    c = (2, 129, 4, 4, 64, "none", 6.0)
    ops = RO.operands(c, 1000 + 129)
    ex = RO.chain(ops, RO.F64)
    below = RO.below_diagonal(2, 129)
    clamped = float(((ex["P"] == RO.EPS) & below).sum()) / float(below.sum())
    assert 0.005 <= clamped <= 0.04, clamped
    assert RO.excluded_share(RO.near_clamp(ex["a"], ex["Z"]), 2, 129) <= RO.MAX_EXCLUDED_SHARE
    ops1 = RO.operands((2, 129, 4, 4, 64, "none", 1.0), 1000 + 129)
    assert not bool(((RO.chain(ops1, RO.F64)["P"] == RO.EPS) & below).any())
