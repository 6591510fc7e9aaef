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

Out of scope (not built here): sampling and generation inside the loop, ``PreferenceRewardModel`` (GPT-2 is CPU plumbing here), the RLHF collators,
``rlhf_grpo_training_loop``, the experimental loop and ``GRPOEvaluator``, RLVR / RPT (their log-prob needs are one call to ``log_probs_per_token``
away; DPO is in ``alignment/dpo/dpo.py``); of the chunked head: a GEMM whose epilogue does the log-sum-exp (a chunk's logits never leaving the CU), skipping the
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
from llm_quest_amd import ops_grpo as O
from llm_quest_amd import ops_pref as OP
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
