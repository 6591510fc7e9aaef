"""CPU-side checks of preference tuning (DPO and the reward model): the public names' signatures and defaults against the reference's
(tests/golden/pref_signatures.json), both collates bit for bit against the fixture, the plain-torch restatement (tests/pref_oracle.py) against the reference's
fp32 and bf16 runs in the fixture with the empty-mask values (NaN, 0, the bias, row S - 1), every refusal by message, the new entry points in header and
binding table with their host-side validation (no launch), and ``CheckpointEvaluator`` on a scripted sequence of calls."""

import inspect
import os
import re

import pytest
import torch

import pref_oracle as PO

BF16, F32, F64, I64 = torch.bfloat16, torch.float32, torch.float64, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mi355_dpo_seq_logprob", "mi355_dpo_seq_logprob_bwd", "mi355_dpo_loss", "mi355_reward_pool_fwd", "mi355_reward_pool_bwd")


@pytest.fixture(scope="module")
def fixture():
    return PO.load_fixture()


def _sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def _modules():
    from llm_quest_amd import config, dataset, utils
    from llm_quest_amd.alignment.dpo import dpo
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    return dpo, grpo_engine, dataset, utils, config


def test_public_names_signatures_and_defaults_match_the_reference(fixture):
    D, G, DS, U, C = _modules()
    want = fixture[1]["signatures"]
    homes = {"DPOLoss": D.DPOLoss, "DPOEvaluator": D.DPOEvaluator, "dpo_training_eval_loop_simple": D.dpo_training_eval_loop_simple,
             "PrefRewardCalculator": G.PrefRewardCalculator, "evaluate_reward_model": G.evaluate_reward_model,
             "reward_model_training_eval_loop_simple": G.reward_model_training_eval_loop_simple, "CheckpointEvaluator": U.CheckpointEvaluator,
             "dpo_collate": DS.dpo_collate, "pref_reward_collate": DS.pref_reward_collate}
    assert len(want) == 21 and {n.split(".")[0] for n in want} == set(homes)
    for name in sorted(want):
        obj = homes[name.split(".")[0]]
        for part in name.split(".")[1:]:
            obj = getattr(obj, part)
        assert _sig(obj) == want[name], name
    assert _sig(D.DPOLoss.forward_from_hidden) == [["self", None], ["batch", None], ["policy_model", None], ["reference_model", None], ["vocab_chunk", "None"]]
    assert _sig(G.PrefRewardCalculator.scores_mean_pooling_from_hidden) == [["hidden_states", None], ["reward_mask", None], ["model_head", None]]
    for n in ("scores_mean_pooling", "hidden_states_mean_pooling", "last_token_score", "scores_mean_pooling_from_hidden"):
        assert isinstance(inspect.getattr_static(G.PrefRewardCalculator, n), staticmethod), n
    assert list(C.rlhf_grpo_checkpoint_dir.parts[-2:]) == fixture[1]["rlhf_grpo_checkpoint_dir_tail"]
    assert issubclass(D.DPOLoss, torch.nn.Module) and G.CheckpointEvaluator is U.CheckpointEvaluator
    assert "PrefRewardCalculator`` pools" in G.__doc__ and "DPO is in" in G.__doc__  # the "Out of scope" list is up to date


def test_collates_equal_the_reference_bit_for_bit(fixture):
    D, G, DS, U, C = _modules()
    t, meta = fixture
    pairs = meta["pairs"]["A"]
    assert [len(p["prompt"]) for p in pairs] == [1, 2, 3, 4]
    for i, kw in enumerate(meta["collate_kwargs"]):
        dpo_kw = dict(kw, mask_prompt_tokens=False) if i == 2 else kw
        for tag, got in (("dpo", DS.dpo_collate(pairs, pad_token_id=PO.PAD, **dpo_kw)), ("rm", DS.pref_reward_collate(pairs, pad_token_id=PO.PAD, **kw))):
            want = {k[len(f"col.{i}.{tag}."):]: v for k, v in t.items() if k.startswith(f"col.{i}.{tag}.")}
            assert list(got) == (["chosen", "rejected", "chosen_mask", "rejected_mask"] + (["chosen_attn_mask", "rejected_attn_mask"] if tag == "rm" else []))
            assert set(got) == set(want)
            for k, v in got.items():
                assert v.dtype == (torch.bool if "mask" in k else I64) and v.device.type == "cpu", (i, tag, k)
                assert v.shape == want[k].shape and torch.equal(v.to(want[k].dtype), want[k]), (i, tag, k)
    assert t["col.1.dpo.chosen"].shape[1] == 6 and t["col.0.dpo.chosen"].shape[1] == 10
    assert int(t["col.2.dpo.chosen_mask"][:, 0].sum()) == 4 and int(t["col.0.dpo.chosen_mask"][:, 0].sum()) == 0
    for name in ("A", "B"):  # the DPO cases' own batches, and the reward masks
        got = DS.dpo_collate(meta["pairs"][name], pad_token_id=PO.PAD)
        for k, v in got.items():
            assert torch.equal(v.to(t[f"{name}.in.{k}"].dtype), t[f"{name}.in.{k}"]), (name, k)
    got = DS.pref_reward_collate(meta["pairs"]["rw"], pad_token_id=PO.PAD)
    assert torch.equal(got["chosen_mask"], t["rw.in.mask_full"].bool()) and torch.equal(got["chosen_attn_mask"], t["rw.in.attn_full"].bool())
    with pytest.raises(ValueError, match="at least one sample"):
        DS.dpo_collate([])


def test_fixture_meets_its_own_conditions(fixture):
    t, meta = fixture
    assert os.path.getsize(os.path.join(PO.GOLDEN, "pref_tiny.safetensors")) < 1 << 20
    for name, spec in PO.DPO_CASES.items():
        assert meta["dpo_cases"][name] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in spec.items()}
        assert meta["seeds"][name] == 0  # the first seed tried met the conditions, so no earlier seed has to be shown to fail
        pairs, inp = PO.dpo_inputs(name, meta["seeds"][name])
        assert pairs == meta["pairs"][name]
        for k, v in inp.items():
            assert torch.equal(v, t[f"{name}.in.{k}"]), (name, k)
        assert tuple(t[f"{name}.in.chosen"].shape) == (spec["b"], spec["S"]) and t[f"{name}.in.pol_chosen_logits"].shape[2] == spec["V"]
        assert len(set(spec["chosen"])) == spec["b"] and len(set(spec["rejected"])) == spec["b"]
        assert bool((t[f"{name}.in.chosen_mask"].sum(1) > 0).all()) and bool((t[f"{name}.in.rejected_mask"].sum(1) > 0).all())
        lp = t[f"{name}.logprobs32"].double()
        for beta, _ in PO.DPO_CONFIGS:
            assert float((beta * ((lp[0] - lp[2]) - (lp[1] - lp[3]))).abs().max()) < 20
    a = PO.DPO_CASES["A"]
    assert a["chosen"][0] > a["rejected"][0] and a["chosen"][1] < a["rejected"][1] and a["prompt"] == (1, 2, 3, 4)
    e = PO.REWARD["empty_seq"]
    assert int(t["rw.in.mask_empty"][e].sum()) == 0 and int(t["rw.in.attn_empty"][e].sum()) == 0 and bool((t["rw.in.mask_full"].sum(1) > 0).all())
    assert tuple(t["rw.in.h32"].shape) == (3, 7, 64) and t["rw.in.h16"].dtype == BF16 and tuple(t["rw.in.w"].shape) == (1, 64)


def _close(got, want, rel, what):
    """Relative L2 over the tensor, NaN positions equal."""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), what
    if bool((~nan).any()):
        d = PO.rel_l2(got[~nan], want[~nan]) if float(want[~nan].double().norm()) > 0 else float(got[~nan].double().abs().max())
        assert d <= rel, (what, d)


@pytest.mark.parametrize("case", ["A", "B"])
def test_restatement_reproduces_the_reference_dpo(fixture, case):
    """fp32 flow: 1e-5 relative L2 (two fp32 computations of one expression); bf16 flow: 2 ** -7, two bf16 ulps, where the order of a sum may differ."""
    t, meta = fixture
    for dtype, tag, rel in ((F32, "32", 1e-5), (BF16, "16", 2.0 ** -7)):
        for masked, key in ((True, "logprobs"), (False, "logprobs_nomask")):
            got = PO.dpo_run(t, case, 0.1, 0.0, dtype, masked)["logprobs"]
            assert got.dtype == t[f"{case}.{key}{tag}"].dtype
            _close(got, t[f"{case}.{key}{tag}"], rel, (case, key, tag))
        for i, (beta, ls) in enumerate(PO.DPO_CONFIGS):
            run = PO.dpo_run(t, case, beta, ls, dtype)
            for k in ("out", "dchosen", "drejected"):
                _close(run[k], t[f"{case}.c{i}.{k}{tag}"], rel * (1 if k == "out" or dtype == F32 else 4), (case, i, k, tag))
            assert float(run["dchosen"][:, -1].abs().max()) == 0.0  # the last position predicts nothing
    assert abs(PO.rel_l2(t[f"{case}.c0.out16"], t[f"{case}.c0.out32"]) - meta["floors"][f"{case}.c0.out"]) <= 1e-9  # the floors are the reference's own


def test_restatement_reproduces_the_reference_pooling(fixture):
    t, meta = fixture
    for head, bias in (("bias", t["rw.in.bias"]), ("nobias", None)):
        for mask_tag in ("full", "empty"):
            for kind in PO.POOLINGS:
                mask = t[f"rw.in.{'attn' if kind == 'lts' else 'mask'}_{mask_tag}"].bool()
                key = f"rw.{kind}.{head}.{mask_tag}"
                for dtype, tag, rel in ((F32, "32", 1e-5), (BF16, "16", 2.0 ** -6)):
                    run = PO.pool_run(kind, t["rw.in.h32" if dtype == F32 else "rw.in.h16"], mask, t["rw.in.w"], bias, t["rw.in.g"], dtype)
                    for k in ("score", "dh", "dw") + (("db",) if bias is not None else ()):
                        _close(run[k].reshape(t[f"{key}.{k}{tag}"].shape), t[f"{key}.{k}{tag}"], rel, (key, k, tag))
                        if dtype == BF16 and float(t[f"{key}.{k}32"].double().norm()) > 0:
                            assert abs(PO.rel_l2(t[f"{key}.{k}16"], t[f"{key}.{k}32"]) - meta["floors"][f"{key}.{k}"]) <= 1e-9


def test_empty_masks_behave_like_the_reference(fixture):
    t, _ = fixture
    e, S = PO.REWARD["empty_seq"], PO.REWARD["S"]
    w, b, h = t["rw.in.w"], t["rw.in.bias"], t["rw.in.h32"]
    for src in ("fixture", "oracle"):
        def score(kind, head):
            if src == "fixture":
                return t[f"rw.{kind}.{head}.empty.score32"]
            mask = t[f"rw.in.{'attn' if kind == 'lts' else 'mask'}_empty"].bool()
            return PO.POOL_FN[kind](h, mask, w, b if head == "bias" else None)
        assert float(score("smp", "bias")[e]) == 0.0 and float(score("smp", "nobias")[e]) == 0.0  # scores mean: 0
        assert float(score("hmp", "bias")[e]) == float(b) and float(score("hmp", "nobias")[e]) == 0.0  # hidden mean: the bias
        want = h[e, S - 1] @ w.reshape(-1)  # last token: row S - 1
        assert abs(float(score("lts", "nobias")[e]) - float(want)) <= 1e-6 and abs(float(score("lts", "bias")[e]) - float(want + b)) <= 1e-6
    for k in ("smp", "hmp"):
        assert float(t[f"rw.{k}.bias.empty.dh32"][e].abs().max()) == 0.0
    assert float(t["rw.lts.bias.empty.dh32"][e, : S - 1].abs().max()) == 0.0 and float(t["rw.lts.bias.empty.dh32"][e, S - 1].abs().max()) > 0.0
    # compute_logprobs: an all-False mask is 0 / 0
    logp = torch.randn(2, 5)
    mask = torch.ones(2, 6, dtype=torch.bool)
    mask[1] = False
    avg = PO.seq_average(logp, mask)
    assert bool(torch.isnan(avg[1])) and bool(torch.isfinite(avg[0]))
    # the denominator is the unshifted sum: six positions, five labels
    assert abs(float(avg[0]) - float(logp[0].sum() / 6)) <= 1e-6


def test_every_refusal_fires_by_message():
    D, G, DS, U, C = _modules()
    from llm_quest_amd import kernels_pref as KP

    loss = D.DPOLoss()
    logits, ids, mask = torch.zeros(2, 5, 16, dtype=BF16), torch.zeros(2, 5, dtype=I64), torch.ones(2, 5, dtype=torch.bool)
    v = torch.zeros(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.compute_logprobs(logits, ids, mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.compute_logprobs(logits, ids)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.compute_loss(v, v, v, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KP.seq_logprob_fwd(torch.zeros(2, 4), mask)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KP.dpo_loss(v, v, v, v, 0.1, 0.0)
    with pytest.raises(TypeError, match="logits must be bf16"):
        loss.compute_logprobs(logits.float(), ids, mask)
    with pytest.raises(TypeError, match=r"inputs must be int64 \[B, S\]"):
        loss.compute_logprobs(logits, ids.int(), mask)
    with pytest.raises(ValueError, match="shapes disagree: attention_mask"):
        loss.compute_logprobs(logits, ids, mask[:, 1:])
    with pytest.raises(ValueError, match="at least two positions"):
        loss.compute_logprobs(logits[:, :1], ids[:, :1])
    with pytest.raises(ValueError, match="shapes disagree: ref_chosen_logprob"):
        loss.compute_loss(v, v, torch.zeros(3), v)
    with pytest.raises(ValueError, match="shapes disagree: pol_rejected_logprob"):
        loss.compute_loss(v, v.double(), v, v)
    with pytest.raises(TypeError, match="attention_mask must be bool, an integer type or a float type"):
        KP.seq_logprob_fwd(torch.zeros(2, 4), torch.ones(2, 5, dtype=torch.complex64))
    batch = {"chosen": ids, "rejected": ids, "chosen_mask": mask, "rejected_mask": mask}

    class NoHead(torch.nn.Module):
        pass

    class WithHead(torch.nn.Module):
        def label_log_probs(self, ids, vocab_chunk=None):
            raise AssertionError("not reached")

    with pytest.raises(TypeError, match=r"policy_model \(NoHead\) has no label_log_probs"):
        loss.forward_from_hidden(batch, NoHead(), WithHead())
    with pytest.raises(TypeError, match=r"reference_model \(NoHead\) has no label_log_probs"):
        loss.forward_from_hidden(batch, WithHead(), NoHead())
    with pytest.raises(ValueError, match="must share one"):
        loss.forward_from_hidden(dict(batch, rejected=ids[:, :4]), WithHead(), WithHead())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss.forward_from_hidden(batch, WithHead(), WithHead())

    P = G.PrefRewardCalculator
    h, m, head = torch.zeros(2, 5, 16, dtype=BF16), torch.ones(2, 5, dtype=torch.bool), torch.nn.Linear(16, 1)
    for fn in (P.hidden_states_mean_pooling, P.last_token_score, P.scores_mean_pooling_from_hidden):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(h, m, head)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(h.float(), m.float(), torch.nn.Linear(16, 1).to(BF16))
        with pytest.raises(TypeError, match="hidden_states must be bf16 or fp32"):
            fn(h.double(), m, head)
        with pytest.raises(ValueError, match=r"hidden_states must be 3-D"):
            fn(h[0], m, head)
        with pytest.raises(ValueError, match="emb_dim must be a multiple of 8"):
            fn(torch.zeros(2, 5, 12, dtype=BF16), m, torch.nn.Linear(12, 1))
        with pytest.raises(ValueError, match="emb_dim must be a multiple of 8, at most 8192"):
            fn(torch.zeros(1, 1, 8200, dtype=BF16), m[:1, :1], torch.nn.Linear(8200, 1))
        with pytest.raises(ValueError, match="shapes disagree: the mask must be"):
            fn(h, m[:, :4], head)
        with pytest.raises(ValueError, match=r"model_head must be a Linear\(16, 1\)"):
            fn(h, m, torch.nn.Linear(16, 2))
        with pytest.raises(TypeError, match="head's weight must be bf16 or fp32"):
            fn(h, m, torch.nn.Linear(16, 1).double())
        with pytest.raises(TypeError, match="model_head must be an nn.Linear"):
            fn(h, m, None)
        with pytest.raises(TypeError, match="must be bool, an integer type or a float type"):
            fn(h, m.to(torch.complex64), torch.nn.Linear(16, 1))
    head = torch.nn.Linear(16, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.scores_mean_pooling(torch.zeros(2, 5, 1), m)
    with pytest.raises(ValueError, match=r"rewards must be the head's output \(b, s, 1\)"):
        P.scores_mean_pooling(torch.zeros(2, 5, 2), m)
    with pytest.raises(TypeError, match="rewards must be bf16 or fp32"):
        P.scores_mean_pooling(torch.zeros(2, 5, 1, dtype=F64), m)
    with pytest.raises(ValueError, match="PrefRewardCalculator.scores_mean_pooling: .*shapes disagree"):
        P.scores_mean_pooling(torch.zeros(2, 5, 1), m[:1])


def test_entry_points_are_declared_bound_and_validate_on_the_host():
    from llm_quest_amd import _lib

    raw = open(os.path.join(ROOT, "include", "mi355_vlm.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} is not declared in include/mi355_vlm.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    for line in ("dpo/dpo.py:59-68", "dpo/dpo.py:88-104", "grpo_engine.py:36-94", ":46-55", ":58-76", ":79-94"):
        assert line in raw, f"the header does not name the reference call site {line}"
    make = open(os.path.join(ROOT, "llm_quest_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpreference\.hip\b", make, flags=re.M) and re.search(r"^USERS_rows_bf16 = .*\bpreference\.o\b", make, flags=re.M)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = torch.zeros(64, dtype=F32)
    p = buf.data_ptr()  # a valid, 16-byte aligned host pointer: never dereferenced, every call below is refused first
    assert p % 16 == 0
    err = lambda: lib.mi355_last_error().decode()
    for B, T in ((1, 1), (0, 4), (4, 0), (4, -1), (1 << 30, 1 << 40)):
        assert lib.mi355_dpo_seq_logprob(B, T, None, None, 0, None, None, None) != 0 and "mi355_dpo_seq_logprob:" in err()
        assert lib.mi355_dpo_seq_logprob_bwd(B, T, None, None, 0, None, None, None) != 0 and "mi355_dpo_seq_logprob_bwd:" in err()
    assert lib.mi355_dpo_seq_logprob(1, 1, p, p, 7, p, p, None) != 0 and "mask dtype" in err()
    assert lib.mi355_dpo_seq_logprob_bwd(1, 1, p, p, -1, p, p, None) != 0 and "mask dtype" in err()
    for n in (1, 0, -3, 1 << 30):
        assert lib.mi355_dpo_loss(n, None, None, None, None, 0.1, 0.0, None, None, None, None) != 0 and "mi355_dpo_loss" in err()
    assert lib.mi355_dpo_loss(2, p, p, p, p, float("nan"), 0.0, p, p, p, None) != 0 and "must be numbers" in err()
    fwd = lambda mode=1, B=1, S=1, E=8, x=p, xdt=0, mask=p, mdt=0, w=p, wdt=0, pooled=p: (mode, B, S, E, x, xdt, mask, mdt, w, wdt, p, p, pooled, p, None)
    bwd = lambda mode=1, B=1, S=1, E=8, mask=p, mdt=0, w=p, wdt=0, dx=p, dw=p, db=p, pooled=p: (mode, B, S, E, p, mask, mdt, p, w, wdt, pooled, dx, 0, dw, db, None)
    for name, call, mk in (("mi355_reward_pool_fwd", lib.mi355_reward_pool_fwd, fwd), ("mi355_reward_pool_bwd", lib.mi355_reward_pool_bwd, bwd)):
        assert call(*mk(mode=4)) != 0 and "unknown mode" in err() and name in err()
        assert call(*mk(mode=-1)) != 0 and "unknown mode" in err()
        for kw in (dict(B=0), dict(S=0), dict(B=1 << 20), dict(S=1 << 40), dict(mask=None)):
            assert call(*mk(**kw)) != 0 and "bad arguments" in err(), kw
        assert call(*mk(mdt=5)) != 0 and "mask dtype" in err()
        assert call(*mk(wdt=2)) != 0 and "bf16 (0) or fp32 (1)" in err()
        for E in (0, 4, 12, 8200, -8):
            assert call(*mk(E=E)) != 0 and "multiple of 8" in err(), E
        assert call(*mk(mode=0, E=8)) != 0 and "(B, S, 1)" in err()
        assert call(*mk(w=None)) != 0 and "head's weight" in err()
        assert call(*mk(w=p + 4)) != 0 and "head's weight" in err()
    assert lib.mi355_reward_pool_fwd(*fwd(x=None)) != 0 and "null pointer" in err()
    assert lib.mi355_reward_pool_fwd(*fwd(x=p + 2)) != 0 and "16-byte aligned" in err()
    assert lib.mi355_reward_pool_fwd(*fwd(pooled=None)) != 0 and "16-byte aligned" in err()
    assert lib.mi355_reward_pool_bwd(*bwd(dx=None, dw=None, db=None)) != 0 and "nothing to compute" in err()
    assert lib.mi355_reward_pool_bwd(*bwd(dx=p + 8)) != 0 and "dx must be 16-byte aligned" in err()
    assert lib.mi355_reward_pool_bwd(*bwd(pooled=None)) != 0 and "needs the pooled rows" in err()
    assert lib.mi355_reward_pool_bwd(*bwd(mode=0, E=1, dx=None)) != 0 and "dx must be non-null" in err()


def test_checkpoint_evaluator_follows_a_scripted_sequence(capsys):
    D, G, DS, U, C = _modules()
    ev = U.CheckpointEvaluator()
    assert (ev.kl_div_threshold, ev.min_reward_threshold, ev.beta, ev.rm_min_accuracy_threshold, ev.rm_min_val_loss_threshold) == (0.5, 6.0, 1.0, 0.9, 0.1)
    assert ev.max_score_grpo == float("-inf") and ev.max_accu_pref_rm == float("-inf")
    # reward model: below the accuracy threshold, above the loss threshold, a first best, an equal one, a better one
    script = [((0.89, 0.05), False), ((0.95, 0.11), False), ((0.92, 0.1), True), ((0.92, 0.01), False), ((0.9, 0.0), False), ((0.93, 0.05), True)]
    for (acc, loss), want in script:
        assert ev.is_rm_accu_best(acc, loss) is want, (acc, loss)
    assert ev.max_accu_pref_rm == 0.93 and ev.max_score_grpo == float("-inf")
    assert capsys.readouterr().out.count("New max accuracy found") == 2
    # GRPO: KL too high, reward too low, a first best (score 6.5 - 0.25), a worse one, then RLVR's method shares the maximum
    ev = U.CheckpointEvaluator(beta=0.5)
    script = [("is_rlhf_grpo_best", (0.6, 9.0), False), ("is_rlhf_grpo_best", (0.1, 5.9), False), ("is_rlhf_grpo_best", (0.5, 6.5), True),
              ("is_rlhf_grpo_best", (0.4, 6.4), False), ("is_rlvr_grpo_best", (0.5, 6.5), False), ("is_rlvr_grpo_best", (0.0, 6.3), True)]
    for method, (kl, reward), want in script:
        assert getattr(ev, method)(kl, reward) is want, (method, kl, reward)
    assert ev.max_score_grpo == 6.3 and "New max score found 6.250" in capsys.readouterr().out
