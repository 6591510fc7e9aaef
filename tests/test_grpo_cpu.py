"""CPU-side checks of the GRPO loss layer: the public names' signatures and defaults against the reference's (tests/golden/grpo_signatures.json), every
refusal by message, the new entry points in header and binding table with their host-side validation (no launch), the fixture's own conditions, the
plain-torch restatement (tests/grpo_oracle.py) against the reference's fp32 and bf16 runs in the fixture, and ``z_scores`` / ``bt_loss``."""

import inspect
import os
import re

import pytest
import torch

import grpo_oracle as GO

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi355_label_logprob_fwd", "mi355_label_logprob_bwd", "mi355_grpo_token_loss", "mi355_grpo_logits_loss", "mi355_grpo_piece")


@pytest.fixture(scope="module")
def fixture():
    return GO.load_fixture()


def _engine():
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    return grpo_engine


def _sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def test_public_names_signatures_and_defaults_match_the_reference(fixture):
    G, want = _engine(), fixture[1]["signatures"]
    names = {"bt_loss", "z_scores", "log_probs_per_token", "log_probs_per_token_optimized", "log_probs_per_seq", "kl_div_per_token", "off_policy_seq_mask",
             "grpo_policy_loss", "GRPOLoss.compute", "GRPOLoss._compute_clipped_surrogate", "GRPOLoss._compute_sapo_surrogate",
             "GRPOLoss._compute_gspo_loss", "GRPOLoss._aggregate"}
    assert set(want) == names
    for name in sorted(names):
        obj = G
        for part in name.split("."):
            obj = getattr(obj, part)
        assert _sig(obj) == want[name], name
    assert _sig(G.grpo_policy_loss) == [["logits", None], ["inputs", None], ["old_logprobs", None], ["reference_logprobs", None], ["advantages", None],
                                        ["loss_mask", None], ["num_samples", None], ["min_clip", None], ["max_clip", None], ["beta", None],
                                        ["max_gen", "1"], ["variant", "'grpo'"], ["unbiased_kl_estimate", "False"], ["off_policy_delta", "None"],
                                        ["inplace", "True"]]
    from llm_quest_amd import config

    assert config.use_phantom_reward is fixture[1]["use_phantom_reward_default"] is False
    assert "consumed" in G.grpo_policy_loss.__doc__.lower() and "bf16" in G.log_probs_per_token_optimized.__doc__


def _operands(B=4, S=5, V=16):
    T = S - 1
    return dict(logits=torch.zeros(B, S, V, dtype=BF16), inputs=torch.zeros(B, S, dtype=I64), old_logprobs=torch.zeros(B, T), reference_logprobs=torch.zeros(B, T),
                advantages=torch.ones(B), loss_mask=torch.ones(B, T, dtype=torch.bool), num_samples=2, min_clip=0.2, max_clip=0.2, beta=0.1)


def test_every_refusal_fires_by_message():
    G = _engine()
    from llm_quest_amd import kernels_grpo as K

    ok = _operands()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.grpo_policy_loss(**ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.log_probs_per_token(ok["logits"], ok["inputs"])
    for fn, args in ((G.log_probs_per_seq, (ok["old_logprobs"], ok["loss_mask"])), (G.kl_div_per_token, (ok["old_logprobs"], ok["reference_logprobs"])),
                     (G.off_policy_seq_mask, (ok["old_logprobs"], ok["advantages"], ok["loss_mask"])),
                     (G.GRPOLoss.compute, (ok["old_logprobs"], ok["advantages"], ok["loss_mask"], 0.2, 0.2, 0.1, ok["old_logprobs"], 2)),
                     (G.GRPOLoss._compute_clipped_surrogate, (ok["old_logprobs"], ok["advantages"].unsqueeze(-1), 0.2, 0.2)),
                     (G.GRPOLoss._compute_sapo_surrogate, (ok["old_logprobs"], ok["advantages"].unsqueeze(-1))),
                     (G.GRPOLoss._compute_gspo_loss, (ok["advantages"], ok["advantages"], 0.2, 0.2)),
                     (G.GRPOLoss._aggregate, (ok["old_logprobs"], ok["loss_mask"], 2, 1, "grpo"))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
    with pytest.raises(TypeError, match="logits must be bf16"):
        G.grpo_policy_loss(**dict(ok, logits=ok["logits"].float()))
    with pytest.raises(TypeError, match="logits must be bf16"):
        G.log_probs_per_token(ok["logits"].float(), ok["inputs"])
    with pytest.raises(TypeError, match=r"inputs must be int64 \[B, S\]"):
        G.grpo_policy_loss(**dict(ok, inputs=ok["inputs"].int()))
    with pytest.raises(TypeError, match=r"inputs must be int64 \[B, S\]"):
        G.log_probs_per_token(ok["logits"], ok["inputs"].flatten())
    with pytest.raises(ValueError, match="shapes disagree"):
        G.log_probs_per_token(ok["logits"], ok["inputs"][:, :-1])
    for key, bad in (("old_logprobs", torch.zeros(4, 5)), ("reference_logprobs", torch.zeros(3, 4)), ("advantages", torch.ones(5)),
                     ("loss_mask", torch.ones(4, 5, dtype=torch.bool)), ("old_logprobs", torch.zeros(4, 4, dtype=F64))):
        with pytest.raises(ValueError, match="shapes disagree"):
            G.grpo_policy_loss(**dict(ok, **{key: bad}))
    for variant in ("grpo", "sapo"):
        with pytest.raises(ValueError, match="not divisible by num_samples"):
            G.grpo_policy_loss(**dict(ok, num_samples=3, variant=variant))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # dapo, dr_grpo and gspo have no groups: 3 is accepted and the call gets to the device check
        G.grpo_policy_loss(**dict(ok, num_samples=3, variant="dapo"))
    with pytest.raises(ValueError, match="Unknown loss type: ppo"):
        G.grpo_policy_loss(**dict(ok, variant="ppo"))
    with pytest.raises(ValueError, match="Unknown loss type: ppo"):
        G.GRPOLoss.compute(ok["old_logprobs"], ok["advantages"], ok["loss_mask"], 0.2, 0.2, 0.1, ok["old_logprobs"], 2, variant="ppo")
    with pytest.raises(ValueError, match="Unknown loss type: gspo"):
        G.GRPOLoss._aggregate(ok["old_logprobs"], ok["loss_mask"], 2, 1, "gspo")
    one = (ok["logits"], ok["inputs"], ok["old_logprobs"], ok["reference_logprobs"], ok["advantages"], ok["loss_mask"], 0.2, 0.2, 0.1, 2)
    with pytest.raises(ValueError, match="one-pass: gspo needs"):
        K.logits_loss(*one, variant="gspo")
    with pytest.raises(ValueError, match="one-pass: the off-policy mask needs"):
        K.logits_loss(*one, use_off_policy_mask=True)
    with pytest.raises(ValueError, match="16-byte rows"):  # the launchers take 16-byte rows only; the public functions pad first
        K.label_logprob_fwd(torch.zeros(2, 3, 7, dtype=BF16), torch.zeros(2, 3, dtype=I64))
    with pytest.raises(ValueError, match="at least two positions"):
        G.grpo_policy_loss(**dict(ok, logits=ok["logits"][:, :1], inputs=ok["inputs"][:, :1], old_logprobs=torch.zeros(4, 0), reference_logprobs=torch.zeros(4, 0),
                                  loss_mask=torch.zeros(4, 0)))


def test_entry_points_are_declared_bound_and_validate_on_the_host():
    from llm_quest_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355_vlm.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/mi355_vlm.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    raw = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    for line in ("grpo_engine.py:397-425", ":492-519", ":522-554", ":557-680", ":1087-1098"):
        assert line in raw, f"the header does not name the reference call site {line}"
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = (torch.zeros(64, dtype=F32))
    p = buf.data_ptr()  # a valid, 16-byte aligned host pointer: never dereferenced, every call below is refused first
    assert p % 16 == 0
    err = lambda: lib.mi355_last_error().decode()
    # null pointers and absurd sizes
    for B, S, V in ((1, 2, 8), (-1, 2, 8), (1, 1, 8), (1, 2, 0), (1 << 40, 1 << 40, 1 << 40)):
        assert lib.mi355_label_logprob_fwd(B, S, V, None, 8, 8, None, None, None, None) != 0 and "mi355_label_logprob_fwd" in err()
        assert lib.mi355_label_logprob_bwd(B, S, V, None, None, 8, 8, None, None, None, 8, 8, None) != 0 and "mi355_label_logprob_bwd" in err()
        assert lib.mi355_grpo_logits_loss(min(B, 1 << 30), S, V, None, 8, 8, None, 8, 8, None, None, None, None, None, 0, 0.2, 0.2, 0.1, 1, 1, 0, 0, 0, None, None,
                                          None, None, None) != 0 and "mi355_grpo_logits_loss" in err()
    for B, T in ((1, 1), (0, 4), (4, -1), (1 << 30, 1 << 40)):
        assert lib.mi355_grpo_token_loss(B, T, None, None, None, None, None, 0, 0.2, 0.2, 0.1, 0.5, 1, 1, 0, 0, 0, None, None, None, None, None, None) != 0
        assert "mi355_grpo_token_loss" in err()
        assert lib.mi355_grpo_piece(1, B, T, None, None, None, None, None, 0, 0.0, 0.0, 0.0, 0, 1, 1, None, None, None, None, None) != 0 and "mi355_grpo_piece" in err()
    # the row pitch: the vector path says what it needs
    assert lib.mi355_label_logprob_fwd(1, 2, 7, p, 16, 7, p, p, p, None) != 0 and "16-byte rows" in err()
    assert lib.mi355_label_logprob_fwd(1, 2, 9, p, 16, 8, p, p, p, None) != 0 and "16-byte rows" in err()  # pitch < V
    assert lib.mi355_label_logprob_fwd(1, 2, 8, p + 2, 16, 8, p, p, p, None) != 0 and "16-byte rows" in err()
    assert lib.mi355_label_logprob_bwd(1, 2, 8, p, p, 16, 8, p, p, p, 24, 8, None) != 0 and "in place" in err()
    # the one-pass entry refuses gspo and the off-policy mask by name; variants, mask dtypes and groups are checked everywhere
    args = lambda variant, opm, mdt=0, ns=1: (2, 3, 8, p, 24, 8, p, 24, 8, p, p, p, p, p, mdt, 0.2, 0.2, 0.1, ns, 1, variant, 0, opm, p, p, p, p, None)
    assert lib.mi355_grpo_logits_loss(*args(4, 0)) != 0 and "gspo" in err() and "two-pass" in err()
    assert lib.mi355_grpo_logits_loss(*args(0, 1)) != 0 and "off-policy mask" in err() and "two-pass" in err()
    assert lib.mi355_grpo_logits_loss(*args(7, 0)) != 0 and "unknown variant" in err()
    assert lib.mi355_grpo_logits_loss(*args(0, 0, mdt=9)) != 0 and "mask dtype" in err()
    assert lib.mi355_grpo_logits_loss(*args(0, 0, ns=3)) != 0 and "multiple of num_samples" in err()
    tl = lambda variant, ns=1, mdt=0: (2, 4, p, p, p, p, p, mdt, 0.2, 0.2, 0.1, 0.5, ns, 1, variant, 0, 0, p, p, p, p, p, None)
    assert lib.mi355_grpo_token_loss(*tl(5)) != 0 and "unknown variant" in err()
    assert lib.mi355_grpo_token_loss(*tl(3, ns=4)) != 0 and "multiple of num_samples" in err()
    assert lib.mi355_grpo_token_loss(*tl(0, mdt=-1)) != 0 and "mask dtype" in err()
    assert lib.mi355_grpo_piece(0, 1, 1, p, p, p, p, p, 0, 0.0, 0.0, 0.0, 0, 1, 1, p, p, p, p, None) != 0 and "unknown op" in err()
    assert lib.mi355_grpo_piece(2, 1, 1, p, p, None, None, None, 0, 0.0, 0.0, 0.0, 0, 1, 1, p, p, None, None, None) != 0 and "misses an operand" in err()
    assert lib.mi355_grpo_piece(5, 1, 1, p, None, None, None, None, 0, 0.0, 0.0, 0.0, 0, 1, 1, p, None, None, None, None) != 0 and "loss mask" in err()
    assert lib.mi355_grpo_piece(9, 1, 1, p, None, None, None, p, 0, 0.0, 0.0, 0.0, 4, 1, 1, p, p, None, p, None) != 0 and "token-level" in err()


def test_fixture_meets_its_own_conditions(fixture):
    t, meta = fixture
    assert os.path.getsize(os.path.join(GO.GOLDEN, "grpo_tiny.safetensors")) < 1 << 20
    assert meta["cases"]["A"] == dict(B=6, S=9, V=40, num_samples=3, dead_seq=4) and {k: meta["cases"]["B"][k] for k in ("B", "S", "V", "num_samples")} == dict(B=2, S=4, V=1000, num_samples=2)
    for case, spec in meta["cases"].items():
        seed = meta["seeds"][case]
        for s in range(seed + 1):  # the stored seed is the FIRST that meets the conditions that depend on the inputs alone
            inp = GO.fixture_inputs(spec["B"], spec["S"], spec["V"], spec["num_samples"], s, dead_seq=spec["dead_seq"])
            if s == seed:
                for k, v in inp.items():
                    assert torch.equal(v, t[f"{case}.in.{k}"].to(v.dtype)), (case, k)
        mask, mg = t[f"{case}.in.mask"].bool(), t[f"{case}.in.mask_gspo"].bool()
        if spec["dead_seq"] is not None:
            assert int(mask[spec["dead_seq"]].sum()) == 0 and int(mg[spec["dead_seq"]].sum()) == 2
        starts = {int(r.float().argmax()) for r in mask if r.any()}
        ends = {int(r.nonzero().max()) for r in mask if r.any()}
        assert len(starts) > 1 and len(ends) > 1, "the masks start and end at different positions"
        delta = meta["delta"][case]
        for m_ in (mask, mg):
            ok, why = GO.conditions(inp, m_, delta)
            assert ok, (case, why)
        assert not bool((t[f"{case}.in.adv"] == 0).any())
        for v, u, m in GO.configs():
            opm = t[f"{case}.{v}.u{u}.m{m}.opm"].bool()
            assert bool(opm.all()) if not m else (bool(opm.any()) and not bool(opm.all())), (case, v, u, m)
    logp = GO.log_probs_per_token(t["A.in.logits"], t["A.in.ids"], F64)
    assert abs(float((t["A.in.old"].double() - logp).std()) - 0.3) < 0.1  # old = policy + 0.3 N(0, 1)


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_reference(fixture, case):
    """fp32 flow: 1e-5 relative on the loss, 1e-4 relative L2 on the logits' gradient; the intermediates likewise; the off-policy mask exactly.  bf16 flow:
    the loss bit for bit (the restatement reduces in the reference's order), and for case A the gradient bit for bit too."""
    t, meta = fixture
    for v, u, m in GO.configs():
        args, key = GO.case_args(t, meta, case, v, u, m)
        o32 = GO.loss_and_grads(*args, F32)
        want = float(t[key + ".loss32"])
        assert abs(float(o32["loss"]) - want) <= 1e-5 * abs(want), (key, float(o32["loss"]), want)
        assert GO.rel_l2(o32["dlogits"][:, :-1], t[key + ".dlogits32"]) <= 1e-4, key
        assert float(o32["dlogits"][:, -1].abs().max()) == 0.0
        assert GO.rel_l2(o32["ratio"], t[key + ".policy_ratio"]) <= 1e-5 and GO.rel_l2(o32["kl"], t[key + ".kl_div"]) <= 1e-5, key
        assert torch.equal(o32["opm"], t[key + ".opm"].bool()), key
        o16 = GO.loss_and_grads(*args, BF16)
        assert o16["loss"].dtype == t[key + ".loss16"].dtype and torch.equal(o16["loss"], t[key + ".loss16"]), (key, float(o16["loss"]), float(t[key + ".loss16"]))
        if case == "A":
            assert torch.equal(o16["dlogits"][:, :-1], t[key + ".dlogits16"]), key
        assert abs(GO.rel_l2(o16["loss"], t[key + ".loss32"]) - meta["floors"][key]["loss"]) <= 1e-9  # the stored floors are those of the reference's own bf16 run


def test_empty_masks_behave_like_the_reference(fixture):
    t, meta = fixture
    for v in GO.TOKEN_LEVEL:
        args, _ = GO.case_args(t, meta, "A", v, 0, 0)
        out = GO.loss_and_grads(*args, F64)
        assert torch.isfinite(out["loss"]) and float(out["dlogits"][4].abs().max()) == 0.0  # sequence 4 contributes nothing
    args, _ = GO.case_args(t, meta, "A", "gspo", 0, 0)
    dead = list(args)
    dead[5] = t["A.in.mask"].bool()
    assert torch.isnan(GO.loss_and_grads(*dead, F64)["loss"])
    assert torch.isnan(GO.log_probs_per_seq(t["A.in.old"], t["A.in.mask"].bool())[4])


def test_z_scores_and_bt_loss_agree_with_the_fixture(fixture):
    G = _engine()
    from llm_quest_amd import config

    t = fixture[0]
    try:
        for phantom in (0, 1):
            config.use_phantom_reward = bool(phantom)
            for key, kw in (("std", {}), ("dr_grpo", {"dr_grpo": "dr_grpo"})):
                got = G.z_scores(t["z.rewards"].clone(), 3, **kw)
                assert torch.allclose(got, t[f"z.p{phantom}.{key}"], rtol=1e-6, atol=1e-7), (phantom, key)
                assert torch.allclose(GO.z_scores(t["z.rewards"], 3, phantom=bool(phantom), **kw), t[f"z.p{phantom}.{key}"], rtol=1e-6, atol=1e-7)
    finally:
        config.use_phantom_reward = False
    with pytest.raises(AssertionError, match="greater than 1"):
        G.z_scores(t["z.rewards"], 1)
    assert torch.allclose(G.bt_loss(t["bt.chosen"], t["bt.rejected"]), t["bt.beta1"], rtol=1e-6)
    assert torch.allclose(G.bt_loss(t["bt.chosen"], t["bt.rejected"], beta=0.5), t["bt.beta05"], rtol=1e-6)
    assert torch.allclose(GO.bt_loss(t["bt.chosen"], t["bt.rejected"], 0.5), t["bt.beta05"], rtol=1e-6)
