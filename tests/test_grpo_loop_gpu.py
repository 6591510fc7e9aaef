"""The RLHF GRPO training loop and its evaluator on a tiny Qwen3 policy / reference and a small hidden-state-pooling reward module: two prompt batches of two
prompts, ``num_samples = 3``, ``max_gen = 6``.  The loop's default EOS / pad id (50 256) lies outside the tiny vocabulary, so every row keeps all its tokens."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TINY = dict(vocab_size=1000, emb_dim=128, n_layers=2, n_heads=4, num_kv_groups=2, head_dim=128, hidden_dim=256, context_length=64, rope_base=1_000_000,
            dtype=BF16, tie_embeddings=True)
NUM_SAMPLES, MAX_GEN, SEED = 3, 6, 21
TOL = 1e-6  # tests/test_grpo_head_gpu.py: the loss from the hidden states against the loss from the logits
VARIANTS = ("grpo", "dapo", "dr_grpo", "sapo", "gspo")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from llm_quest_amd import _lib, generate
    from llm_quest_amd.alignment.rlhf_grpo import grpo_engine

    _lib.load()
    return grpo_engine, generate, torch.device("cuda", 0)


class Reward(torch.nn.Module):
    """Token embeddings as the hidden states, the head on their masked mean (``PrefRewardCalculator.hidden_states_mean_pooling``).  ``bias=10`` lifts every
    score above ``CheckpointEvaluator``'s reward threshold (the checkpoint test); the loss tests keep 0: rewards of 10 that differ by 0.05 lose six digits in
    ``rewards - mean``, and the z-scores of a group then sum to 1e-5 instead of fp32 rounding."""

    def __init__(self, bias=0.0):
        super().__init__()
        torch.manual_seed(5)
        self.emb = torch.nn.Embedding(TINY["vocab_size"], 64, dtype=BF16)
        self.head = torch.nn.Linear(64, 1, dtype=BF16)
        with torch.no_grad():
            self.head.bias.fill_(bias)

    def forward(self, ids, attn_mask=None, reward_mask=None):
        from llm_quest_amd.alignment.rlhf_grpo.grpo_engine import PrefRewardCalculator

        return PrefRewardCalculator.hidden_states_mean_pooling(self.emb(ids), reward_mask, self.head)


class LogitsOnly(torch.nn.Module):
    """A policy that offers logits and nothing else (no ``label_log_probs``, ``forward_hidden`` or ``out_head``): the loop's fallback path."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    @property
    def trf_blocks(self):
        return self.inner.trf_blocks

    def forward(self, x, attn_mask=None, kv_cache=None, position_ids=None):
        return self.inner(x, attn_mask=attn_mask, kv_cache=kv_cache, position_ids=position_ids)


def make_policy(dev, wrap=False):
    from llm_quest_amd.qwen.qwen3.qwen3_model import Qwen3Model

    torch.manual_seed(0)
    m = Qwen3Model(dict(TINY))
    return (LogitsOnly(m) if wrap else m).to(dev)


def make_loaders(E, dev):
    g = torch.Generator().manual_seed(2)
    batches = [[torch.randint(10, 1000, (n,), generator=g).tolist() for n in lens] for lens in ((5, 8), (7, 4), (6, 6))]
    coll = [E.rlhf_grpo_prompt_collator(b, pad_token_id=3, device=dev) for b in batches]  # the prompts' padding must be a token the embedding holds
    return coll[:2], coll[2:]


class Recorder:
    """Wraps the two loss entries of the module and keeps what they returned."""

    def __init__(self, E, monkeypatch):
        self.hidden, self.logits = [], []
        for name, store in (("grpo_policy_loss_from_hidden", self.hidden), ("grpo_policy_loss", self.logits)):
            fn = getattr(E, name)
            monkeypatch.setattr(E, name, lambda *a, _fn=fn, _store=store, **k: self._keep(_fn(*a, **k), _store))

    @staticmethod
    def _keep(loss, store):
        store.append(float(loss.detach()))
        return loss


def run_loop(E, G, dev, policy, reference, variant="grpo", num_epoch=1, num_grad_updates=1, loaders=None, reward_bias=0.0, **kw):
    train, val = loaders or make_loaders(E, dev)
    opt = torch.optim.SGD(policy.parameters(), lr=1e-2)
    E.rlhf_grpo_training_loop(train, val, policy, reference, Reward(reward_bias).to(dev), opt, num_epoch, NUM_SAMPLES, num_grad_updates, TINY, dev, max_gen=MAX_GEN, beta=1.0,
                              loss_variant=variant, rng=G.SampleRNG(SEED), **kw)


def test_first_step_loss_is_the_logits_paths_and_parameters_move(env, monkeypatch):
    """``num_grad_updates=1``, ``beta=1``, variant "grpo": the first step's loss is what ``log_probs_per_token`` -> ``GRPOLoss.compute`` give on the same collated
    batch, and it is 0: the ratio is 1, the KL 0, and the z-scores of a group sum to zero.  The parameters move."""
    E, G, dev = env
    rec = Recorder(E, monkeypatch)
    policy, reference = make_policy(dev), make_policy(dev)
    before = {n: p.detach().clone() for n, p in policy.named_parameters()}
    run_loop(E, G, dev, policy, reference, evaluation=False)
    assert len(rec.hidden) == 2 and not rec.logits, "a Qwen3Model takes the hidden-state path, one loss per step"
    assert sum(int(not torch.equal(p.detach(), before[n])) for n, p in policy.named_parameters()) > 0
    assert all(bool(torch.isfinite(p.float()).all()) for p in policy.parameters())
    # the same first batch by hand, on the logits
    fresh, reward = make_policy(dev), Reward().to(dev).eval()
    batch = make_loaders(E, dev)[0][0]
    rep = lambda k: batch[k].repeat_interleave(NUM_SAMPLES, dim=0)
    fresh.eval()
    resp = G.generate_batched_rollouts(rep("padded_prompts"), fresh, MAX_GEN, TINY["context_length"], top_k=20, temp=1.0, last_real=rep("last_real_pos"), device=dev,
                                       attention_mask=rep("prompt_masks"), rng=G.SampleRNG(SEED))
    col = E.batched_responses_collator(resp, prompt_masks=rep("prompt_masks"), device=dev)
    ids, attn, mask = col["padded_responses"], col["attn_masks"], col["reward_masks"][:, 1:]
    assert bool(mask.any(dim=1).all()), "every row has live tokens"
    with torch.no_grad():
        old = E.log_probs_per_token(fresh(ids, attn), ids)
        adv = E.z_scores(reward(ids, attn_mask=attn, reward_mask=col["reward_masks"]).float(), NUM_SAMPLES, dr_grpo="grpo")
    fresh.train()
    pol = E.log_probs_per_token(fresh(ids, attn), ids)
    want = float(E.GRPOLoss.compute(policy_ratio=torch.exp(pol - old), advantages=adv, loss_mask=mask, min_clip=0.2, max_clip=0.2, beta=1.0,
                                    kl_div=E.kl_div_per_token(pol, old), num_samples=NUM_SAMPLES, variant="grpo").detach())
    print(f"\n[loop] first step: loss {rec.hidden[0]:.3e}, on the logits by hand {want:.3e}")
    assert abs(rec.hidden[0] - want) <= TOL * max(1.0, abs(want))
    assert abs(rec.hidden[0]) <= TOL and abs(want) <= TOL


def test_reference_takes_the_policys_weights_at_every_epoch(env):
    E, G, dev = env
    policy, reference = make_policy(dev), make_policy(dev)
    with torch.no_grad():
        for p in reference.parameters():
            p.add_(1.0)
    train, val = make_loaders(E, dev)
    seen = []

    class Loader(list):
        def __iter__(self):  # the loop walks the loader right after the epoch's synchronisation
            seen.append(all(torch.equal(a, b) for a, b in zip(policy.state_dict().values(), reference.state_dict().values())))
            return super().__iter__()

    run_loop(E, G, dev, policy, reference, num_epoch=2, loaders=(Loader(train[:1]), val), evaluation=False)
    assert seen == [True, True]
    assert not all(torch.equal(a, b) for a, b in zip(policy.state_dict().values(), reference.state_dict().values())), "the policy has moved on since"


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_runs_two_steps(env, monkeypatch, variant):
    E, G, dev = env
    rec = Recorder(E, monkeypatch)
    policy = make_policy(dev)
    run_loop(E, G, dev, policy, make_policy(dev), variant=variant, num_grad_updates=2, evaluation=False, unbiased_kl_estimate=variant == "dapo")
    assert len(rec.hidden) == 4 and all(x == x and abs(x) < float("inf") for x in rec.hidden), rec.hidden
    assert all(bool(torch.isfinite(p.float()).all()) for p in policy.parameters())


def test_a_policy_without_the_hidden_path_takes_the_logits(env, monkeypatch):
    """The same loop on a wrapper that offers logits alone: ``log_probs_per_token`` / ``grpo_policy_loss``; its losses match the hidden-state path's."""
    E, G, dev = env
    rec = Recorder(E, monkeypatch)
    run_loop(E, G, dev, make_policy(dev), make_policy(dev), evaluation=False)
    hidden = list(rec.hidden)
    run_loop(E, G, dev, make_policy(dev, wrap=True), make_policy(dev, wrap=True), evaluation=False)
    assert len(rec.logits) == 2 and len(rec.hidden) == 2, "the wrapper never reaches the hidden-state entry"
    print(f"\n[loop] hidden-state path {hidden}, logits path {rec.logits}")
    assert abs(hidden[0] - rec.logits[0]) <= TOL * max(1.0, abs(hidden[0]))


def test_evaluator_and_checkpoint(env, monkeypatch, tmp_path):
    """``GRPOEvaluator.evaluate`` returns the four reference keys, its KL is 0 when the policy is the reference, "rlvr" calls the caller's calculator; the loop
    saves a checkpoint under ``config.rlhf_grpo_checkpoint_dir`` when the score improves."""
    E, G, dev = env
    from llm_quest_amd import config

    policy, reference = make_policy(dev), make_policy(dev)
    train, val = make_loaders(E, dev)
    reward = Reward(10.0).to(dev)
    out = E.GRPOEvaluator.evaluate(train, val, policy, reference, TINY, dev, MAX_GEN, reward_model=reward, eval_num_samples=2, rng=G.SampleRNG(SEED))
    assert set(out) == {"train_reward", "train_kl_div", "val_reward", "val_kl_div"} and all(isinstance(v, float) for v in out.values())
    assert abs(out["train_kl_div"]) <= 1e-6 and abs(out["val_kl_div"]) <= 1e-6 and out["val_reward"] > 6.0
    assert policy.training
    sampled = E.GRPOEvaluator.evaluate(train, val, policy, reference, TINY, dev, MAX_GEN, reward_model=reward, sampling_params={"top_k": 20, "temp": 1.0},
                                       eval_num_batches=1, rng=G.SampleRNG(SEED), sync_every=4)
    assert abs(sampled["val_kl_div"]) <= 1e-6
    calls = []

    def calculator(responses, answers):
        calls.append((tuple(responses.shape), list(answers)))
        return torch.full((responses.shape[0],), 2.0, device=responses.device)

    for b, a in zip(train + val, (["a", "b"], ["c", "d"], ["e", "f"])):
        b["answers"] = a
    rlvr = E.GRPOEvaluator.evaluate(train, val, policy, reference, TINY, dev, MAX_GEN, evaluation_type="rlvr", reward_calculator=calculator, eval_num_samples=2)
    assert rlvr["train_reward"] == 2.0 and rlvr["val_reward"] == 2.0 and len(calls) == 3 and calls[0][1] == ["a", "a", "b", "b"] and calls[0][0][0] == 4
    with torch.no_grad():  # move the policy away from the reference: the KL must see it
        for p in policy.parameters():
            p.mul_(1.05)
    moved = E.GRPOEvaluator.evaluate(train, val, policy, reference, TINY, dev, MAX_GEN, reward_model=reward)
    assert moved["val_kl_div"] > 1e-6

    monkeypatch.setattr(config, "rlhf_grpo_checkpoint_dir", tmp_path / "ckpt")
    policy = make_policy(dev)
    run_loop(E, G, dev, policy, make_policy(dev), loaders=(train, val), evaluation=True, eval_freq=1, eval_batches=1, reward_bias=10.0)
    saved = sorted(os.listdir(tmp_path / "ckpt"))
    assert saved and all(n.startswith("best_checkpoint_") and n.endswith(".pt") for n in saved), saved
    state = torch.load(tmp_path / "ckpt" / saved[-1], map_location="cpu")
    assert set(state) == set(policy.state_dict())
