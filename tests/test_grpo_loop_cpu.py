"""CPU checks of the RLHF GRPO loop's host side: the reference's names and parameter lists, the prompt collator against the fixture, the refusals."""

import inspect
import json
import os

import pytest
import torch
from safetensors.torch import load_file

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXTENSIONS = [["rng", "None"], ["sync_every", "1"], ["vocab_chunk", "None"]]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "rollout_signatures.json")) as f:
        meta = json.load(f)
    return load_file(os.path.join(GOLDEN, "rollout_tiny.safetensors")), meta


def sig(fn):
    return [[n, None if p.default is inspect.Parameter.empty else repr(p.default)] for n, p in inspect.signature(fn).parameters.items()]


def test_the_loop_is_importable_under_the_references_names():
    from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import GRPOEvaluator, batched_responses_collator, rlhf_grpo_prompt_collator, rlhf_grpo_training_loop

    assert callable(rlhf_grpo_training_loop) and callable(rlhf_grpo_prompt_collator) and callable(batched_responses_collator)
    assert callable(GRPOEvaluator.evaluate) and callable(GRPOEvaluator._compute_grpo_metrics)


def test_signatures_are_the_references_plus_the_listed_extensions(fixture):
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as E

    ref = fixture[1]["signatures"]["reference"]
    assert sig(E.rlhf_grpo_prompt_collator) == ref["rlhf_grpo_prompt_collator"]
    assert sig(E.batched_responses_collator) == ref["batched_responses_collator"]
    assert sig(E.rlhf_grpo_training_loop) == ref["rlhf_grpo_training_loop"] + EXTENSIONS
    assert sig(E.GRPOEvaluator.evaluate) == ref["GRPOEvaluator.evaluate"] + EXTENSIONS
    assert sig(E.GRPOEvaluator._compute_grpo_metrics) == ref["GRPOEvaluator._compute_grpo_metrics"] + EXTENSIONS


def test_prompt_collator_is_bit_equal_to_the_fixture(fixture):
    from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import rlhf_grpo_prompt_collator

    t, meta = fixture
    for k, m in meta["prompts"].items():
        prompts = [list(p) for p in m["prompts"]]
        out = rlhf_grpo_prompt_collator(prompts, pad_token_id=m["pad_token_id"], custom_max_length=m["custom_max_length"])
        assert prompts == m["prompts"], "the caller's lists stay untouched"
        assert set(out) == {"padded_prompts", "prompt_masks", "last_real_pos"}
        assert out["prompt_masks"].dtype == torch.bool and out["padded_prompts"].dtype == torch.int64 and out["last_real_pos"].dtype == torch.int64
        for n, v in out.items():
            want = t[f"prompts.{k}.{n}"]
            assert torch.equal(v.to(want.dtype), want), (k, n)


def test_refusals_without_a_gpu():
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as E

    resp, pm = torch.zeros(2, 6, dtype=torch.long), torch.ones(2, 3, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.batched_responses_collator(resp, pm, device="cpu")
    with pytest.raises(ValueError, match="prompt_masks"):
        E.batched_responses_collator(resp, torch.ones(3, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="int64"):
        E.batched_responses_collator(resp.int(), pm)
    with pytest.raises(ValueError, match="EOS ids"):
        E.batched_responses_collator(resp, pm, eos_ids=list(range(9)))
    with pytest.raises(ValueError, match="reward_model is required"):
        E.GRPOEvaluator.evaluate(None, None, None, None, {}, "cuda", 4)
    with pytest.raises(ValueError, match="reward_calculator is required"):
        E.GRPOEvaluator.evaluate(None, None, None, None, {}, "cuda", 4, evaluation_type="rlvr")
    with pytest.raises(ValueError, match="Invalid evaluation type"):
        E.GRPOEvaluator.evaluate(None, None, None, None, {}, "cuda", 4, evaluation_type="other")


def test_module_docstring_names_what_is_in_and_what_is_out():
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as E

    doc = E.__doc__
    assert "rlhf_grpo_training_loop" in doc and "GRPOEvaluator" in doc and "Out of scope" in doc
    out = doc[doc.index("Out of scope"):]
    assert "rlhf_grpo_training_loop`` and" not in out and "grpo_training_loop_variant_experimental" in out and "VerifiableRewardCalculator" in out
