"""The GRPO loss layer (reference: llm_quest/alignment/rlhf_grpo/grpo_engine.py) on the HIP kernels of csrc/grpo.hip.

The functions carry the reference's names, parameter order and defaults, so a training loop written against it (:1082-1111) runs unchanged:
``log_probs_per_token`` -> the ratio -> ``kl_div_per_token`` -> ``GRPOLoss.compute`` -> ``backward()``.  ``grpo_policy_loss`` is this project's own
entry for those lines: one call from the logits to the scalar loss, in ONE pass over the logits where the mathematics allows it.

What differs from the reference, on purpose:

* Logits are bf16 device tensors and every log-prob is computed and returned in fp32.  The reference takes ``log_softmax`` in the logits' own dtype
  (bf16 there), a loss of precision that is not reproduced; ``log_probs_per_token_optimized`` is the same kernel, so its bf16 caveat does not apply.
* The per-token functions take and return fp32 ``[B, T]`` device tensors; host tensors are refused (there is no CPU fallback), except in ``z_scores``
  and ``bt_loss``, which work on ``B`` numbers in plain torch on either device.
* ``loss_mask`` may be bool, an integer type or a float type holding 0 or 1.

Like the reference: a sequence whose mask is empty contributes 0 in the token-level variants; an empty mask gives NaN in ``log_probs_per_seq`` and so
in GSPO.

From the hidden states (this project's own names, csrc/grpo_head.hip): ``log_probs_per_token_from_hidden`` and ``grpo_policy_loss_from_hidden`` take the
final-normed hidden states and the model's output head instead of logits and walk the head in vocabulary chunks, so the (B, S, vocab_size) logits -- held
three times per batch by a loop on the functions above: the policy's and, under no-grad, the old and the reference policy's -- never exist.
``Qwen3Model.label_log_probs`` is the one call a loop makes per policy.  The log-probs are those of the bf16 logits the head's GEMM would have written.

The reward model's side (csrc/preference.hip): ``PrefRewardCalculator`` pools a backbone's hidden states into one score per sequence with the head's
``Linear(emb_dim, 1)`` folded into the kernel -- one pass over the hidden states, fp32 accumulation, fp32 ``(b,)`` scores, the gradients of the hidden states,
the weight and the bias from its backward; ``scores_mean_pooling_from_hidden`` is this project's own name for the reference reward model's default pooling
without the ``(b, s, 1)`` intermediate and without an N = 1 GEMM.  ``evaluate_reward_model`` and ``reward_model_training_eval_loop_simple`` are the
reference's loops; the models here are bf16 themselves, so the loops carry no autocast context.  The reward model is any module called as
``reward_model(ids, attn_mask=..., reward_mask=...)`` that returns ``(b,)`` scores (the reference's GPT-2-based ``PreferenceRewardModel`` is not built).

The RLHF loop (csrc/sampling.hip for its rollouts): ``rlhf_grpo_prompt_collator``, ``batched_responses_collator``, ``rlhf_grpo_training_loop`` and
``GRPOEvaluator`` carry the reference's names, parameter order and defaults.  The rollouts come from ``generate.generate_batched_rollouts`` (one sampling
launch per token that also keeps the loop's books, no ``torch.cat`` per token); the response masks are one integer kernel; a model that offers
``label_log_probs`` (or ``forward_hidden`` and ``out_head``) takes the vocabulary-chunked head, so the (B, S, vocab_size) logits do not exist three times per
batch, any other model takes ``log_probs_per_token`` / ``grpo_policy_loss`` on its logits.  Trailing keyword extensions: ``rng`` (a ``generate.SampleRNG``),
``sync_every`` (how often the rollout loop reads the device) and ``vocab_chunk``.  The old / reference log-probs and the rewards run under
``torch.no_grad()`` where upstream has ``inference_mode``, for the reason given at ``evaluate_reward_model``.

Out of scope (not built here): ``PreferenceRewardModel`` (GPT-2 is CPU plumbing here), the experimental loop
(``grpo_training_loop_variant_experimental``), RLVR / RPT and ``VerifiableRewardCalculator`` (string and tokenizer work; their log-prob needs are one call
to ``log_probs_per_token`` away; DPO is in ``alignment/dpo/dpo.py``), left-padded rollouts, hipGraph capture of the sampled step; of the chunked head: a GEMM
whose epilogue does the log-sum-exp (a chunk's logits never leaving the CU), skipping the
rows whose ``loss_mask`` is 0, and a ``label_log_probs`` on the model classes other than ``Qwen3Model`` (the two functions themselves are
model-agnostic: any ``forward_hidden`` and output head will do).
"""

import os

import torch
import torch.nn.functional as F

from llm_quest_amd import _lib as L
from llm_quest_amd import config
from llm_quest_amd import kernels_grpo as K
from llm_quest_amd import kernels_grpo_head as KH
from llm_quest_amd import kernels_pref as KP
from llm_quest_amd import kernels_sample as KS
from llm_quest_amd import ops_grpo as O
from llm_quest_amd import ops_pref as OP
from llm_quest_amd.generate import generate_batched_rollouts
from llm_quest_amd.utils import CheckpointEvaluator

_TOKEN_LEVEL = ("grpo", "dapo", "dr_grpo", "sapo")


def bt_loss(chosen_logits, rejected_logits, beta=1.0):
    """Bradley-Terry loss of the reward model: mean over the batch of -log sigmoid(beta (chosen - rejected)).  ``B`` numbers: plain torch."""
    return -F.logsigmoid(beta * (chosen_logits - rejected_logits)).mean()


class PrefRewardCalculator:
    """The ways to turn a reward model's output into one score per sequence, fp32 (b,), each one kernel (csrc/preference.hip):

    - ``scores_mean_pooling``: the masked mean of the head's per-token scores (b, s, 1);
    - ``hidden_states_mean_pooling``: the head on the masked mean of the hidden states;
    - ``last_token_score``: the head on the hidden state of the last real token;
    - ``scores_mean_pooling_from_hidden``: ``scores_mean_pooling(model_head(hidden_states), reward_mask)`` from the hidden states themselves.

    ``hidden_states`` are bf16 or fp32 (b, s, emb_dim) on the device, emb_dim a multiple of 8 up to 8 192; ``model_head`` is an ``nn.Linear(emb_dim, 1)`` with or
    without bias, its parameters bf16 or fp32 whatever the hidden states are; the masks are (b, s) of 0 / 1 in bool, an integer type or a float type.  Rows
    whose mask is 0 are not read, and their gradient is exact zeros."""

    @staticmethod
    def scores_mean_pooling(rewards, reward_mask):
        """``sum(rewards * reward_mask) / max(count, 1)``; an empty mask gives 0."""
        _pool_operands("PrefRewardCalculator.scores_mean_pooling", rewards, reward_mask, None, 0)
        return OP.RewardPoolFn.apply(rewards, reward_mask, None, None, 0)

    @staticmethod
    def hidden_states_mean_pooling(hidden_states, reward_mask, model_head):
        """``model_head(sum(hidden_states * reward_mask) / max(count, 1))``; an empty mask gives the head's bias."""
        w, b = _pool_operands("PrefRewardCalculator.hidden_states_mean_pooling", hidden_states, reward_mask, model_head, 1)
        return OP.RewardPoolFn.apply(hidden_states, reward_mask, w, b, 1)

    @staticmethod
    def last_token_score(hidden_states, attention_mask, model_head):
        """``model_head(hidden_states[b, attention_mask[b].sum() - 1])``; a count of 0 selects row ``s - 1`` (upstream's index -1)."""
        w, b = _pool_operands("PrefRewardCalculator.last_token_score", hidden_states, attention_mask, model_head, 2)
        return OP.RewardPoolFn.apply(hidden_states, attention_mask, w, b, 2)

    @staticmethod
    def scores_mean_pooling_from_hidden(hidden_states, reward_mask, model_head):
        """``sum_t reward_mask (hidden_states_t . w + bias) / max(count, 1)``: the per-token scores are never written; an empty mask gives 0."""
        w, b = _pool_operands("PrefRewardCalculator.scores_mean_pooling_from_hidden", hidden_states, reward_mask, model_head, 3)
        return OP.RewardPoolFn.apply(hidden_states, reward_mask, w, b, 3)


def _pool_operands(what, hidden, mask, model_head, mode):
    """The refusals shared by the four pooling functions, host side first; returns the head's (weight, bias)."""
    w = b = None
    if mode != 0:
        w, b = getattr(model_head, "weight", None), getattr(model_head, "bias", None)
        if not isinstance(w, torch.Tensor):
            raise TypeError(f"{what}: model_head must be an nn.Linear(emb_dim, 1)")
    try:
        B, S, E = KP.check_hidden(hidden, mask, mode, "rewards" if mode == 0 else "hidden_states")
        KP.mask_operand(mask, (B, S), "the mask")
        if mode != 0:
            KP.check_head(w, b, E)
    except (TypeError, ValueError) as e:
        raise type(e)(f"{what}: {e}") from None
    _device_only(hidden, mask, w, b)
    return w, b


def evaluate_reward_model(val_loader, reward_model, eval_num_batches=None, beta=1.0):
    """(average Bradley-Terry loss per batch, share of pairs whose chosen score exceeds the rejected one) over the first ``eval_num_batches`` batches of
    ``val_loader`` (None: all of it), in eval mode and without gradients; the model is put back in train mode."""
    total_loss, correct, count = 0.0, 0, 0
    num_batches_to_eval = min(eval_num_batches, len(val_loader)) if eval_num_batches else len(val_loader)
    reward_model.eval()
    with torch.no_grad():  # upstream: inference_mode; the models here keep lazily built device buffers, which must stay usable by the next training step
        for i, batch in enumerate(val_loader):
            if i >= num_batches_to_eval:
                break
            pref_rewards = reward_model(batch["chosen"], attn_mask=batch["chosen_attn_mask"], reward_mask=batch["chosen_mask"])
            rej_rewards = reward_model(batch["rejected"], attn_mask=batch["rejected_attn_mask"], reward_mask=batch["rejected_mask"])
            total_loss += bt_loss(pref_rewards, rej_rewards, beta=beta).item()
            correct += (pref_rewards > rej_rewards).sum().item()
            count += pref_rewards.shape[0]
    reward_model.train()
    return total_loss / num_batches_to_eval, correct / count


def reward_model_training_eval_loop_simple(
    train_loader,
    val_loader,
    reward_model,
    optimizer,
    num_epoch,
    eval_freq,
    eval_num_batches=None,
    beta=1.0,
):
    """Train ``reward_model`` on ``pref_reward_collate`` batches with the Bradley-Terry loss.  Every ``eval_freq`` steps: the interval's training loss and
    accuracy, ``evaluate_reward_model`` on ``eval_num_batches`` batches, and -- when ``CheckpointEvaluator.is_rm_accu_best`` says so -- the model's
    ``state_dict`` saved under ``config.rlhf_grpo_checkpoint_dir``.  Returns the tracked metrics."""
    step = 0
    interval_loss, interval_correct, interval_count = 0.0, 0, 0
    tracking = {"train_losses": [], "val_losses": [], "train_acc": [], "val_acc": []}
    chkp_eval = CheckpointEvaluator()
    reward_model.train()
    for epoch in range(1, num_epoch + 1):
        for batch in train_loader:
            step += 1
            pref_rewards = reward_model(batch["chosen"], attn_mask=batch["chosen_attn_mask"], reward_mask=batch["chosen_mask"])
            rej_rewards = reward_model(batch["rejected"], attn_mask=batch["rejected_attn_mask"], reward_mask=batch["rejected_mask"])
            loss = bt_loss(pref_rewards, rej_rewards, beta=beta)
            loss.backward()
            optimizer.step()
            optimizer.zero_grad()
            interval_loss += loss.item()
            interval_correct += (pref_rewards > rej_rewards).sum().item()
            interval_count += pref_rewards.shape[0]
            if step % eval_freq == 0:
                train_loss = interval_loss / eval_freq
                train_acc = interval_correct / interval_count if interval_count > 0 else 0.0
                val_loss, val_acc = evaluate_reward_model(val_loader, reward_model, eval_num_batches, beta=beta)
                tracking["train_losses"].append(train_loss)  # upstream declares the two training lists and leaves them empty
                tracking["train_acc"].append(train_acc)
                tracking["val_losses"].append(val_loss)
                tracking["val_acc"].append(val_acc)
                print(
                    f"Epoch: {epoch}, Step: {step} |",
                    f"T. loss: {train_loss:.5f}, V. loss: {val_loss:.5f} |",
                    f"T. acc: {train_acc * 100:.2f}%, V. acc: {val_acc * 100:.2f}%",
                )
                if chkp_eval.is_rm_accu_best(val_acc, val_loss):
                    os.makedirs(config.rlhf_grpo_checkpoint_dir, exist_ok=True)
                    name = f"best_rm_checkpoint_{step}_accu_{chkp_eval.max_accu_pref_rm:.3f}_loss_{val_loss:.3f}.pt"
                    torch.save(reward_model.state_dict(), os.path.join(config.rlhf_grpo_checkpoint_dir, name))
                interval_loss, interval_correct, interval_count = 0.0, 0, 0
    return tracking


def z_scores(rewards, num_samples, dr_grpo=None):
    """Advantages by outcome supervision: the rewards (B,) standardised inside each group of ``num_samples``; with ``dr_grpo == "dr_grpo"`` only
    centred.  ``config.use_phantom_reward`` adds one reward of 0 to every group before its statistics.  ``B`` numbers: plain torch."""
    rewards = rewards.view(-1, num_samples)
    if config.use_phantom_reward:
        augmented = torch.cat([rewards, torch.zeros(rewards.shape[0], 1, device=rewards.device)], dim=1)
    else:
        augmented = rewards
    mean = augmented.mean(dim=1, keepdim=True)
    if dr_grpo == "dr_grpo":
        return (rewards - mean).view(-1)
    if not config.use_phantom_reward:
        assert num_samples > 1, "num_samples must be greater than 1 to get a relative comparison"
    std = augmented.std(dim=1, keepdim=True)
    return ((rewards - mean) / (std + 1e-8)).view(-1)


def _device_only(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("llm_quest_amd GRPO functions run only on an MI355X (HIP) device; got a CPU tensor.  There is no CPU fallback for this path.")


def _vector_logits(logits):
    """The logits as the kernels can address them: as they are, or -- a row pitch that is no multiple of 8 elements -- through the padded copy cross
    entropy uses (its backward copies the gradient back)."""
    if K.rows_are_vector_ready(logits):
        return logits
    from llm_quest_amd.engine import _pad_rows

    B, S, V = logits.shape
    return _pad_rows(logits.reshape(B * S, V)).unflatten(0, (B, S))


def log_probs_per_token(logits, inputs):
    """The log-probability of each label: ``logits`` bf16 (B, S, vocab_size) on the device, ``inputs`` int64 (B, S).  Returns fp32 (B, S - 1):
    ``logits[b, s, inputs[b, s + 1]] - logsumexp(logits[b, s, :])``, all arithmetic in fp32 (not in bf16 as upstream).  One autograd node: the backward
    writes the logits' gradient into a fresh buffer -- the logits stay the caller's.  ``S == 1`` gives an empty (B, 0) result without a launch."""
    B, S, V = K.check_logits_ids(logits, inputs, "log_probs_per_token")
    _device_only(logits, inputs)
    if S == 1:
        return torch.empty((B, 0), dtype=torch.float32, device=logits.device)
    return O.LabelLogProbFn.apply(_vector_logits(logits), inputs, False)


def log_probs_per_token_optimized(logits, inputs):
    """``log_probs_per_token`` under the reference's other name: the same kernel.  Upstream this form (label logit minus logsumexp) is the one not to
    use in bf16; here the subtraction runs in fp32 on an fp32 logsumexp, so that caveat does not apply."""
    return log_probs_per_token(logits, inputs)


def log_probs_per_seq(logprobs_per_token, loss_mask):
    """The masked mean log-prob of each sequence, fp32 (B,); an empty mask gives NaN, as upstream."""
    _device_only(logprobs_per_token, loss_mask)
    return O.SeqMeanFn.apply(logprobs_per_token, loss_mask)


def kl_div_per_token(policy_logprobs, reference_logprobs, policy_ratio=None):
    """The k3 estimate of the KL per token, ``exp(ref - pol) - (ref - pol) - 1``; with ``policy_ratio`` (the unbiased estimate of DeepSeek-V3.2) times
    that ratio, which then receives a gradient too."""
    _device_only(policy_logprobs, reference_logprobs, policy_ratio)
    return O.KlDivFn.apply(policy_logprobs, reference_logprobs, policy_ratio)


def off_policy_seq_mask(kl_div_per_token, advantages, loss_mask, delta=0.5):
    """The off-policy sequence mask of DeepSeek-V3.2, bool (B, 1): True unless the advantage is negative and the masked mean KL exceeds ``delta``."""
    _device_only(kl_div_per_token, advantages, loss_mask)
    return O.off_policy(kl_div_per_token, advantages, loss_mask, delta)[1]


class GRPOLoss:
    """The GRPO-family losses: hard-clipped surrogate (GRPO, DAPO, Dr. GRPO), soft gate (SAPO), sequence level (GSPO)."""

    @staticmethod
    def compute(
        policy_ratio,
        advantages,
        loss_mask,
        min_clip,
        max_clip,
        beta,
        kl_div,
        num_samples,
        max_gen=1,
        variant="grpo",
        off_policy_mask=None,
    ):
        if variant == "gspo":
            return GRPOLoss._compute_gspo_loss(policy_ratio, advantages, min_clip, max_clip, off_policy_mask)
        if variant not in _TOKEN_LEVEL:
            raise ValueError(f"Unknown loss type: {variant}")
        _device_only(policy_ratio, advantages, loss_mask, kl_div, off_policy_mask)
        return O.RatioLossFn.apply(policy_ratio, kl_div, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen, variant, off_policy_mask)

    @staticmethod
    def _compute_clipped_surrogate(policy_ratio, advantages_broadcast, min_clip, max_clip):
        _device_only(policy_ratio, advantages_broadcast)
        return O.SurrogateFn.apply(policy_ratio, advantages_broadcast, min_clip, max_clip, False)

    @staticmethod
    def _compute_sapo_surrogate(policy_ratio, advantages_broadcast, temp_pos_tokens=1.0, temp_neg_tokens=1.05):
        _device_only(policy_ratio, advantages_broadcast)
        return O.SurrogateFn.apply(policy_ratio, advantages_broadcast, temp_pos_tokens, temp_neg_tokens, True)

    @staticmethod
    def _compute_gspo_loss(masked_policy_ratio, advantages, min_clip, max_clip, off_policy_mask=None):
        _device_only(masked_policy_ratio, advantages, off_policy_mask)
        return O.GspoLossFn.apply(masked_policy_ratio, advantages, min_clip, max_clip, off_policy_mask)

    @staticmethod
    def _aggregate(loss_per_token, loss_mask, num_samples, max_gen, variant):
        if variant not in _TOKEN_LEVEL:
            raise ValueError(f"Unknown loss type: {variant}")
        _device_only(loss_per_token, loss_mask)
        return O.AggregateFn.apply(loss_per_token, loss_mask, num_samples, max_gen, variant)


def grpo_policy_loss(logits, inputs, old_logprobs, reference_logprobs, advantages, loss_mask, num_samples, min_clip, max_clip, beta, max_gen=1,
                     variant="grpo", unbiased_kl_estimate=False, off_policy_delta=None, inplace=True):
    """The scalar GRPO loss of the policy's ``logits`` bf16 (B, S, vocab_size) for ``inputs`` int64 (B, S): what a training loop calls instead of the
    reference's lines 1082-1111 (log-probs, ratio, KL, ``GRPOLoss.compute``).  ``old_logprobs`` / ``reference_logprobs`` fp32 (B, S - 1) come from
    ``log_probs_per_token`` under ``torch.no_grad()``; ``advantages`` fp32 (B,); ``off_policy_delta``: the threshold of the off-policy sequence
    mask, None for no mask.

    With a token-level ``variant``, no off-policy mask and grad mode on, one kernel reads each logits row once, forms its loss term and overwrites it
    with d loss / d logits.  THE LOGITS ARE CONSUMED with ``inplace=True`` (the default, as the LM-head loss does): after the call they hold their own
    gradient, which ``backward()`` hands to the model.  ``inplace=False`` leaves them untouched and keeps the gradient in a fresh buffer.  GSPO and the
    off-policy mask need a per-sequence quantity first and take the two-pass path (label log-probs, per-token chain, log-prob backward -- in place under
    the same flag).  In no-grad mode only the forward runs.  ``backward()`` reads its incoming gradient once on the host to skip a pass over the logits
    when it is exactly 1."""
    B, S, V = K.check_logits_ids(logits, inputs, "grpo_policy_loss")
    K.check_scalars(B, num_samples, max_gen, variant)
    if S < 2:
        raise ValueError("grpo_policy_loss: the sequences need at least two positions")
    T = S - 1
    old, ref = K._tok(old_logprobs, "old_logprobs", B, T), K._tok(reference_logprobs, "reference_logprobs", B, T)
    adv = K._adv(advantages, B)
    K.mask_operand(loss_mask, B, T)
    _device_only(logits, inputs, old, ref, adv, loss_mask)
    grad = torch.is_grad_enabled() and logits.requires_grad
    args = (min_clip, max_clip, beta, num_samples, max_gen, variant, bool(unbiased_kl_estimate))
    if not grad:
        logp, _ = K.label_logprob_fwd(_vector_logits(logits.detach()), inputs)
        return K.token_loss(logp, old, ref, adv, loss_mask, *args, delta=off_policy_delta, want_grad=False)[0]
    lg = _vector_logits(logits)
    if variant in _TOKEN_LEVEL and off_policy_delta is None:
        return O.LogitsLossFn.apply(lg, inputs, old, ref, adv, loss_mask, *args, bool(inplace))[0]
    logp = O.LabelLogProbFn.apply(lg, inputs, bool(inplace))
    return O.TokenLossFn.apply(logp, old, ref, adv, loss_mask, *args, off_policy_delta)[0]


# ------------------------------------------------------------------------------------------------ from the hidden states: no logits in memory
def _head_weight(out_head, what):
    weight = getattr(out_head, "weight", None)
    if not isinstance(weight, torch.Tensor):
        raise TypeError(f"{what}: out_head must be the model's output head, a module with a bf16 ``weight`` (vocab_size, emb_dim)")
    return weight


def log_probs_per_token_from_hidden(hidden, out_head, inputs, vocab_chunk=None):
    """What ``log_probs_per_token(out_head(hidden), inputs)`` defines, fp32 (B, S - 1), without the logits: ``hidden`` bf16 (B, S, emb_dim) are the
    final-normed hidden states (``forward_hidden``), ``out_head`` the model's output head (a module with a bf16 ``weight`` (vocab_size, emb_dim) that its
    arena knows; tied or not).  The head is walked in chunks of ``vocab_chunk`` columns (a positive multiple of 8; None: ``KH.head_chunks``' default): one
    GEMM writes a chunk's bf16 logits, a row kernel folds them into an online log-sum-exp, and the backward recomputes each chunk -- 4 / 3 of the head's
    GEMM work for (B, S, vocab_size) less memory, three times per batch.  ``S == 1`` gives an empty (B, 0) result without a launch."""
    weight = _head_weight(out_head, "log_probs_per_token_from_hidden")
    B, S, D, V = KH.check_head(hidden, weight, inputs, "log_probs_per_token_from_hidden")
    KH.head_chunks(B * S, V, vocab_chunk)
    _device_only(hidden, weight, inputs)
    if S == 1:
        return torch.empty((B, 0), dtype=torch.float32, device=hidden.device)
    if not (torch.is_grad_enabled() and (hidden.requires_grad or weight.requires_grad)):
        return KH.head_logprob_fwd(hidden.detach(), weight.detach(), inputs, vocab_chunk)[0]
    return O.HeadLogProbFn.apply(hidden, inputs, out_head, weight, vocab_chunk)


def grpo_policy_loss_from_hidden(hidden, out_head, inputs, old_logprobs, reference_logprobs, advantages, loss_mask, num_samples, min_clip, max_clip, beta,
                                 max_gen=1, variant="grpo", unbiased_kl_estimate=False, off_policy_delta=None, vocab_chunk=None):
    """``grpo_policy_loss`` from the policy's hidden states instead of its logits: ``log_probs_per_token_from_hidden``, then the per-token chain as one
    node.  All five variants and the off-policy mask take this one path: every per-sequence quantity is known before the backward walks the head's
    chunks.  Nothing is consumed; the other operands are those of ``grpo_policy_loss``.  In no-grad mode only the forward runs."""
    weight = _head_weight(out_head, "grpo_policy_loss_from_hidden")
    B, S, D, V = KH.check_head(hidden, weight, inputs, "grpo_policy_loss_from_hidden")
    KH.head_chunks(B * S, V, vocab_chunk)
    K.check_scalars(B, num_samples, max_gen, variant)
    if S < 2:
        raise ValueError("grpo_policy_loss_from_hidden: the sequences need at least two positions")
    T = S - 1
    old, ref = K._tok(old_logprobs, "old_logprobs", B, T), K._tok(reference_logprobs, "reference_logprobs", B, T)
    adv = K._adv(advantages, B)
    K.mask_operand(loss_mask, B, T)
    _device_only(hidden, weight, inputs, old, ref, adv, loss_mask)
    args = (min_clip, max_clip, beta, num_samples, max_gen, variant, bool(unbiased_kl_estimate))
    logp = log_probs_per_token_from_hidden(hidden, out_head, inputs, vocab_chunk)
    if not logp.requires_grad:
        return K.token_loss(logp, old, ref, adv, loss_mask, *args, delta=off_policy_delta, want_grad=False)[0]
    return O.TokenLossFn.apply(logp, old, ref, adv, loss_mask, *args, off_policy_delta)[0]


# ------------------------------------------------------------------------------------------------ the RLHF loop: collators, training loop, evaluator
def rlhf_grpo_prompt_collator(prompts, pad_token_id=50256, custom_max_length=None, device=torch.device("cpu")):
    """Pad a list of prompts (lists of token ids) to one length on the right: ``padded_prompts`` int64 (b, max_len), ``prompt_masks`` bool of the same
    shape (False on the padding) and ``last_real_pos`` int64 (b,), the index of each prompt's last real token.  ``custom_max_length`` truncates.  Host list
    work."""
    longest = max(len(sample) for sample in prompts)
    if custom_max_length is not None:
        prompts = [sample[:custom_max_length] for sample in prompts]
        longest = min(longest, custom_max_length)
    padded = [sample + [pad_token_id] * (longest - len(sample)) for sample in prompts]
    masks = [[True] * len(sample) + [False] * (longest - len(sample)) for sample in prompts]
    last = [len(sample) - 1 for sample in prompts]
    return {
        "padded_prompts": torch.tensor(padded).to(device),
        "prompt_masks": torch.tensor(masks, dtype=torch.bool).to(device),
        "last_real_pos": torch.tensor(last, dtype=torch.long).to(device),
    }


def batched_responses_collator(responses, prompt_masks, device="cuda", eos_ids=50256, pad_token_id=50256):
    """The masks of a batch of rollouts, one integer kernel (csrc/sampling.hip): ``responses`` int64 (b, prompt_len + generated) and ``prompt_masks`` bool
    (b, prompt_len) on the device.  ``attn_masks``: the prompt as ``prompt_masks`` has it, the response up to and including its first EOS / pad token
    (upstream's ``cumsum <= 1``: every column before the SECOND stop token, which in a rollout directly follows the first); ``reward_masks``: the same with
    the prompt cleared; ``padded_responses``: the responses themselves.  Trailing all-pad columns (``sync_every > 1``) are masked like any padding."""
    attn, reward = KS.response_masks(responses, prompt_masks, eos_ids, pad_token_id)
    return {"padded_responses": responses.to(device), "reward_masks": reward.to(device), "attn_masks": attn.to(device)}


def _policy_label_log_probs(model, ids, attn_mask, vocab_chunk):
    """fp32 (B, S - 1) label log-probs of ``model``: through the vocabulary-chunked head where the model offers it, else from its logits."""
    if _has_hidden_path(model):
        return log_probs_per_token_from_hidden(model.forward_hidden(ids, attn_mask), model.out_head, ids, vocab_chunk)
    return log_probs_per_token(logits=model(ids, attn_mask), inputs=ids)


def _has_hidden_path(model):
    if type(model).__name__ == "Qwen3MoEModel":  # its blocks keep auxiliary state per forward; the logits path is the one it is tested on
        return False
    return callable(getattr(model, "forward_hidden", None)) and isinstance(getattr(getattr(model, "out_head", None), "weight", None), torch.Tensor)


def _build_lazy_buffers(*models):
    """The models here build device buffers on their first forward: that must not happen inside the rollouts' ``inference_mode``."""
    for model in models:
        for m in model.modules() if isinstance(model, torch.nn.Module) else ():
            build = getattr(m, "_build_arenas", None)
            if callable(build):
                build()


def rlhf_grpo_training_loop(
    train_loader,
    val_loader,
    policy_model,
    reference_model,
    reward_model,
    optimizer,
    num_epoch,
    num_samples,
    num_grad_updates,
    policy_config,
    device,
    max_gen=35,
    min_clip_eps=0.2,
    max_clip_eps=0.2,
    beta=1.0,
    unbiased_kl_estimate=False,
    evaluation=True,
    eval_freq=None,
    eval_batches=None,
    eval_num_samples=1,
    kl_div_threshold=0.5,
    loss_variant="grpo",
    save_checkpoint=True,
    rng=None,
    sync_every=1,
    vocab_chunk=None,
):
    """The GRPO training loop (reference grpo_engine.py:1014-1151).  Per epoch the reference model takes the policy's weights; per batch of
    ``rlhf_grpo_prompt_collator`` prompts: every prompt ``num_samples`` times (``repeat_interleave``), rollouts with ``top_k=20, temp=1.0``
    (``generate_batched_rollouts``), the masks (``batched_responses_collator``), the old and the reference log-probs and the reward model's scores without
    gradients, ``z_scores``, then ``num_grad_updates`` updates of the policy on the GRPO loss of ``loss_variant``.  Every ``eval_freq`` steps
    ``GRPOEvaluator.evaluate`` runs and, when ``CheckpointEvaluator.is_rlhf_grpo_best`` says so, the policy's ``state_dict`` is saved under
    ``config.rlhf_grpo_checkpoint_dir``.  Returns None; ``policy_model`` is trained in place.

    ``rng`` / ``sync_every`` go to the rollouts, ``vocab_chunk`` to the chunked head (module docstring)."""
    reward_model.eval()
    reference_model.eval()
    chkp_eval = CheckpointEvaluator(kl_div_threshold=kl_div_threshold, beta=beta)
    _build_lazy_buffers(policy_model, reference_model, reward_model)
    hidden = _has_hidden_path(policy_model)

    step = 0
    for epoch in range(1, num_epoch + 1):
        reference_model.load_state_dict(policy_model.state_dict())

        for batch in train_loader:
            step += 1
            policy_model.eval()  # for every new batch the policy and the old policy are the same
            dup_prompts = batch["padded_prompts"].repeat_interleave(num_samples, dim=0)
            dup_prompts_masks = batch["prompt_masks"].repeat_interleave(num_samples, dim=0)
            last_real_pos = batch["last_real_pos"].repeat_interleave(num_samples, dim=0)

            responses = generate_batched_rollouts(
                input_tensor=dup_prompts,
                model=policy_model,
                attention_mask=dup_prompts_masks,
                max_gen=max_gen,
                context_length=policy_config["context_length"],
                top_k=20,
                top_p=None,
                min_p=None,
                temp=1.0,
                last_real=last_real_pos,
                device=device,
                rng=rng,
                sync_every=sync_every,
            )  # (batch_size * num_samples, max_prompt_len + generated): (B, S)
            collated_batch = batched_responses_collator(responses, prompt_masks=dup_prompts_masks.to(device), device=device)
            ids, attn_masks = collated_batch["padded_responses"], collated_batch["attn_masks"]
            loss_mask = collated_batch["reward_masks"][:, 1:]  # the token positions the log-probs belong to

            with torch.no_grad():
                old_logprobs = _policy_label_log_probs(policy_model, ids, attn_masks, vocab_chunk)
                reference_logprobs = _policy_label_log_probs(reference_model, ids, attn_masks, vocab_chunk)
                rewards = reward_model(ids, attn_mask=attn_masks, reward_mask=collated_batch["reward_masks"])  # (B,)
            advantages = z_scores(rewards.float(), num_samples, dr_grpo=loss_variant)

            policy_model.train()
            cum_grpo_loss = 0.0
            for grad_step in range(num_grad_updates):
                args = (ids, old_logprobs, reference_logprobs, advantages, loss_mask, num_samples, min_clip_eps, max_clip_eps, beta)
                kwargs = dict(variant=loss_variant, unbiased_kl_estimate=unbiased_kl_estimate)
                if hidden:
                    grpo_loss_batch = grpo_policy_loss_from_hidden(policy_model.forward_hidden(ids, attn_masks), policy_model.out_head, *args,
                                                                   vocab_chunk=vocab_chunk, **kwargs)
                else:
                    grpo_loss_batch = grpo_policy_loss(policy_model(ids, attn_masks), *args, **kwargs)
                optimizer.zero_grad()
                grpo_loss_batch.backward()
                optimizer.step()
                cum_grpo_loss += grpo_loss_batch.item()
            avg_grpo_loss = cum_grpo_loss / num_grad_updates

            if evaluation and eval_freq is not None and (step % eval_freq == 0):
                eval_metrics = GRPOEvaluator.evaluate(
                    train_loader=train_loader,
                    val_loader=val_loader,
                    policy_model=policy_model,
                    reference_model=reference_model,
                    evaluation_type="rlhf",
                    reward_model=reward_model,
                    policy_config=policy_config,
                    device=device,
                    max_gen=max_gen,
                    eval_num_samples=eval_num_samples,
                    eval_num_batches=eval_batches,
                    rng=rng,
                    sync_every=sync_every,
                    vocab_chunk=vocab_chunk,
                )
                print(
                    f"Step {step} | "
                    f"Avg GRPO Loss: {avg_grpo_loss:.4f} | "
                    f"T. Rwd: {eval_metrics['train_reward']:.4f}, T. KL Div: {eval_metrics['train_kl_div']:.4f} | "
                    f"V. Rwd: {eval_metrics['val_reward']:.4f}, V. KL Div: {eval_metrics['val_kl_div']:.4f}"
                )
                if save_checkpoint and chkp_eval.is_rlhf_grpo_best(eval_metrics["val_kl_div"], eval_metrics["val_reward"]):
                    os.makedirs(config.rlhf_grpo_checkpoint_dir, exist_ok=True)
                    save_path = os.path.join(config.rlhf_grpo_checkpoint_dir, f"best_checkpoint_{step}_score_{chkp_eval.max_score_grpo:.3f}.pt")
                    torch.save(policy_model.state_dict(), save_path)


class GRPOEvaluator:
    """The average reward and KL divergence of the policy on the training and the validation prompts, for RLHF (a reward model) and RLVR (the caller's
    ``reward_calculator``)."""

    @staticmethod
    def _compute_grpo_metrics(
        loader,
        policy_model,
        reference_model,
        policy_config,
        device,
        max_gen,
        eval_num_samples,
        eval_num_batches,
        evaluation_type="rlhf",
        reward_model=None,
        reward_calculator=None,
        eos_ids=50256,
        pad_id=50256,
        sampling_params=None,
        rng=None,
        sync_every=1,
        vocab_chunk=None,
    ):
        total_reward = 0.0
        total_kl_div = 0.0
        num_batches_to_eval = min(eval_num_batches, len(loader)) if eval_num_batches else len(loader)
        for i, batch in enumerate(loader):
            if i >= num_batches_to_eval:
                break
            dup_prompts = batch["padded_prompts"].repeat_interleave(eval_num_samples, dim=0)
            dup_prompts_masks = batch["prompt_masks"].repeat_interleave(eval_num_samples, dim=0)
            last_real_pos = batch["last_real_pos"].repeat_interleave(eval_num_samples, dim=0)
            responses = generate_batched_rollouts(
                input_tensor=dup_prompts,
                model=policy_model,
                attention_mask=dup_prompts_masks,
                max_gen=max_gen,
                context_length=policy_config["context_length"],
                last_real=last_real_pos,
                device=device,
                eos_ids=eos_ids,
                pad_id=pad_id,
                rng=rng,
                sync_every=sync_every,
                **(sampling_params if sampling_params is not None else {}),
            )
            collated_batch = batched_responses_collator(responses, prompt_masks=dup_prompts_masks.to(device), device=device)
            ids, attn_masks = collated_batch["padded_responses"], collated_batch["attn_masks"]
            loss_mask = collated_batch["reward_masks"][:, 1:]
            policy_logprobs = _policy_label_log_probs(policy_model, ids, attn_masks, vocab_chunk)
            reference_logprobs = _policy_label_log_probs(reference_model, ids, attn_masks, vocab_chunk)
            if evaluation_type == "rlhf":
                rewards = reward_model(ids, attn_mask=attn_masks, reward_mask=collated_batch["reward_masks"])
            elif evaluation_type == "rlvr":
                correct_answers = [ans for ans in batch["answers"] for _ in range(eval_num_samples)]
                rewards = reward_calculator(ids, correct_answers)
            mean_batch_rewards = rewards.float().mean()
            # the masked mean KL per sequence on the device (the k3 kernel, then the sequence average of kernels_pref), one read per batch
            kl_div = kl_div_per_token(policy_logprobs, reference_logprobs)
            seq_mask = torch.cat([torch.zeros_like(loss_mask[:, :1]), loss_mask], dim=1)  # the average takes the unshifted (B, T + 1) form
            mean_kl_per_seq, den = KP.seq_logprob_fwd(kl_div, seq_mask)
            mean_batch_kl_div = torch.where(den > 0, mean_kl_per_seq, torch.zeros_like(mean_kl_per_seq)).mean()  # upstream clamps an empty mask's count to 1: 0
            total_reward += mean_batch_rewards.item()
            total_kl_div += mean_batch_kl_div.item()
        return {"reward": total_reward / num_batches_to_eval, "kl_div": total_kl_div / num_batches_to_eval}

    @staticmethod
    def evaluate(
        train_loader,
        val_loader,
        policy_model,
        reference_model,
        policy_config,
        device,
        max_gen,
        evaluation_type="rlhf",
        reward_model=None,
        reward_calculator=None,
        eval_num_samples=1,
        eval_num_batches=None,
        eos_ids=50256,
        pad_id=50256,
        sampling_params=None,
        rng=None,
        sync_every=1,
        vocab_chunk=None,
    ):
        """{"train_reward", "train_kl_div", "val_reward", "val_kl_div"} of the policy over ``eval_num_batches`` batches of each loader (None: all), with
        ``eval_num_samples`` rollouts per prompt (``sampling_params``: top_k / top_p / min_p / temp of the rollouts, greedy by default), in eval mode and
        without gradients; the policy is put back in train mode.  ``evaluation_type``: "rlhf" scores with ``reward_model``, "rlvr" calls
        ``reward_calculator(padded_responses, correct_answers)`` with the batch's ``answers`` repeated per sample."""
        if evaluation_type == "rlhf":
            if reward_model is None:
                raise ValueError("reward_model is required for RLHF evaluation")
            reward_model.eval()
        elif evaluation_type == "rlvr":
            if reward_calculator is None:
                raise ValueError("reward_calculator is required for RLVR evaluation")
        else:
            raise ValueError(f"Invalid evaluation type: {evaluation_type}")
        policy_model.eval()
        reference_model.eval()
        _build_lazy_buffers(policy_model, reference_model, reward_model)
        with torch.no_grad():  # upstream: inference_mode (see evaluate_reward_model)
            metrics = [
                GRPOEvaluator._compute_grpo_metrics(loader, policy_model, reference_model, policy_config, device, max_gen, eval_num_samples, eval_num_batches,
                                                    evaluation_type=evaluation_type, reward_model=reward_model, reward_calculator=reward_calculator,
                                                    eos_ids=eos_ids, pad_id=pad_id, sampling_params=sampling_params, rng=rng, sync_every=sync_every,
                                                    vocab_chunk=vocab_chunk)
                for loader in (train_loader, val_loader)
            ]
        policy_model.train()
        return {"train_reward": metrics[0]["reward"], "train_kl_div": metrics[0]["kl_div"], "val_reward": metrics[1]["reward"],
                "val_kl_div": metrics[1]["kl_div"]}
