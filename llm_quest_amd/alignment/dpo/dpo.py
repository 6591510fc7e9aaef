"""Direct Preference Optimization (reference: llm_quest/alignment/dpo/dpo.py) on the HIP kernels of csrc/grpo.hip, csrc/grpo_head.hip and
csrc/preference.hip.

``DPOLoss``, ``DPOEvaluator`` and ``dpo_training_eval_loop_simple`` carry the reference's names, parameter order and defaults, so a script written against it
runs unchanged.  A step is: the label log-probs of the policy (with gradient) and of the reference model (without) on the chosen and the rejected sequences, their
masked average per sequence, and the loss of Rafailov et al. with the label smoothing of conservative DPO.  Three kernels beside the label log-probs: the
sequence average and its backward (``mi355_dpo_seq_logprob``), and ONE launch that gives the loss, both reward means and both policy gradients
(``mi355_dpo_loss``).  No reduction runs in torch ops and no value is read back to the host on the way to ``loss.backward()``.

What differs from the reference, on purpose:

* Logits are bf16 device tensors; the log-probs, their averages and the loss are computed and returned in fp32 (upstream: ``log_softmax`` in the logits' own
  dtype).  This is the deviation the GRPO layer documents (``grpo_engine.log_probs_per_token``).
* ``attention_mask`` may be bool, an integer type or a float type holding 0 or 1.  Host tensors are refused: there is no CPU fallback.
* ``forward`` runs each model once on the concatenated (2b, s) batch instead of twice on (b, s): the same numbers, one rounding less in the bf16 gradients.
* ``forward_from_hidden`` is this project's own: the same triple without the (2b, s, vocab_size) logits, which ``forward`` holds once per model.

Like the reference: the denominator of the masked average is the sum of the UNSHIFTED mask over all ``s`` positions, not clamped -- a sequence whose mask is
all False gives NaN; the rewards are detached and not scaled by ``beta``.
"""

import torch
import torch.nn as nn

from llm_quest_amd import ops_pref as OP
from llm_quest_amd.alignment.rlhf_grpo import grpo_engine as G

_NO_CPU = "llm_quest_amd DPO functions run only on an MI355X (HIP) device; got a CPU tensor.  There is no CPU fallback for this path."


def _device_only(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _seq_average(logp, attention_mask, what):
    """The masked average of fp32 label log-probs (b, s - 1) under the unshifted mask (b, s) or None; fp32 (b,)."""
    B, T = logp.shape
    if T < 1:
        raise ValueError(f"{what}: the sequences need at least two positions")
    if attention_mask is not None and tuple(attention_mask.shape) != (B, T + 1):
        raise ValueError(f"{what}: shapes disagree: attention_mask must be {(B, T + 1)}, got {tuple(attention_mask.shape)}")
    _device_only(logp, attention_mask)
    return OP.SeqLogProbFn.apply(logp, attention_mask)


class DPOLoss(nn.Module):
    """The DPO loss from the log-probs of a policy and a reference model on chosen and rejected responses.

    ``beta``: the temperature of the implicit reward.  ``label_smoothing``: the share of preference labels assumed to be flipped (conservative DPO,
    Mitchell 2023, eq. 3); 0 is the original loss."""

    def __init__(self, beta=0.1, label_smoothing=0.0):
        super().__init__()
        self.beta = beta
        self.label_smoothing = label_smoothing

    def compute_logprobs(self, logits, inputs, attention_mask=None):
        """The average label log-prob of each sequence, fp32 (b,): ``logits`` bf16 (b, s, v) on the device, ``inputs`` int64 (b, s), ``attention_mask``
        (b, s) or None.  With a mask: ``sum_t logp[b, t] mask[b, t + 1] / sum_s mask[b, s]``; without: the mean over the ``s - 1`` labels."""
        B, S, V = G.K.check_logits_ids(logits, inputs, "DPOLoss.compute_logprobs")
        if S < 2:
            raise ValueError("DPOLoss.compute_logprobs: the sequences need at least two positions")
        if attention_mask is not None and tuple(attention_mask.shape) != (B, S):
            raise ValueError(f"DPOLoss.compute_logprobs: shapes disagree: attention_mask must be {(B, S)}, got {tuple(attention_mask.shape)}")
        _device_only(logits, inputs, attention_mask)
        return _seq_average(G.log_probs_per_token(logits, inputs), attention_mask, "DPOLoss.compute_logprobs")

    def compute_loss(self, pol_chosen_logprob, pol_rejected_logprob, ref_chosen_logprob, ref_rejected_logprob):
        """(loss, chosen_rewards, rejected_rewards), 0-d fp32, from the four (b,) vectors of ``compute_logprobs``: with
        ``l = (pol_chosen - ref_chosen) - (pol_rejected - ref_rejected)`` the loss is the batch mean of
        ``-logsigmoid(beta l) (1 - label_smoothing) - logsigmoid(-beta l) label_smoothing``; the rewards are the batch means of the two log-ratios, detached."""
        vecs = (pol_chosen_logprob, pol_rejected_logprob, ref_chosen_logprob, ref_rejected_logprob)
        n = pol_chosen_logprob.numel()
        for name, v in zip(("pol_chosen_logprob", "pol_rejected_logprob", "ref_chosen_logprob", "ref_rejected_logprob"), vecs):
            if v.dtype != torch.float32 or v.dim() != 1 or v.shape[0] != n or n < 1:
                raise ValueError(f"DPOLoss.compute_loss: shapes disagree: {name} must be fp32 ({n},), got {v.dtype} {tuple(v.shape)}")
        _device_only(*vecs)
        return OP.DpoLossFn.apply(pol_chosen_logprob, pol_rejected_logprob, ref_chosen_logprob.detach(), ref_rejected_logprob.detach(), self.beta,
                                  self.label_smoothing)

    def forward(self, batch, policy_model, reference_model):
        """The loss of a ``dpo_collate`` batch through the logits.  Chosen and rejected come padded to one length and rows are independent, so each model
        runs ONCE on the concatenated (2b, s) batch: upstream's four passes give the same numbers, but their two policy backwards add up in the bf16
        gradient buffers (a rounding per pass, 2e-3 of the gradient on a tiny Qwen3).  Sides of different shapes take upstream's four passes."""
        chosen, rejected = batch["chosen"], batch["rejected"]
        if chosen.shape != rejected.shape:
            pol = [self.compute_logprobs(logits=policy_model(batch[k]), inputs=batch[k], attention_mask=batch[f"{k}_mask"]) for k in ("chosen", "rejected")]
            with torch.no_grad():
                ref = [self.compute_logprobs(logits=reference_model(batch[k]), inputs=batch[k], attention_mask=batch[f"{k}_mask"])
                       for k in ("chosen", "rejected")]
            return self.compute_loss(pol[0], pol[1], ref[0], ref[1])
        return self._loss_of_pairs(batch, lambda model, ids, mask: self.compute_logprobs(logits=model(ids), inputs=ids, attention_mask=mask), policy_model,
                                   reference_model)

    def forward_from_hidden(self, batch, policy_model, reference_model, vocab_chunk=None):
        """``forward`` without the logits: each model reads its label log-probs through ``model.label_log_probs`` (the output head walked in chunks of
        ``vocab_chunk`` columns) on ONE concatenated (2b, s) batch -- ``dpo_collate`` pads chosen and rejected to a common length, and rows are
        independent; the reference model runs under ``torch.no_grad()``."""
        for name, model in (("policy_model", policy_model), ("reference_model", reference_model)):
            if not callable(getattr(model, "label_log_probs", None)):
                raise TypeError(f"DPOLoss.forward_from_hidden: {name} ({type(model).__name__}) has no label_log_probs(ids, vocab_chunk=...); use forward, "
                                f"or a model that reads its label log-probs from the hidden states (Qwen3Model)")
        chosen, rejected = batch["chosen"], batch["rejected"]
        if chosen.shape != rejected.shape or chosen.dim() != 2:
            raise ValueError(f"DPOLoss.forward_from_hidden: shapes disagree: chosen {tuple(chosen.shape)} and rejected {tuple(rejected.shape)} must share one "
                             f"(b, s), as dpo_collate pads them")
        return self._loss_of_pairs(batch, lambda model, ids, mask: _seq_average(model.label_log_probs(ids, vocab_chunk=vocab_chunk), mask,
                                                                                "DPOLoss.forward_from_hidden"), policy_model, reference_model)

    def _loss_of_pairs(self, batch, seq_logprobs, policy_model, reference_model):
        """``compute_loss`` of ``seq_logprobs(model, ids, mask)`` on the concatenated (2b, s) batch: the policy with gradient, the reference model without."""
        _device_only(batch["chosen"], batch["rejected"], batch["chosen_mask"], batch["rejected_mask"])
        b = batch["chosen"].shape[0]
        ids = torch.cat([batch["chosen"], batch["rejected"]], dim=0)
        mask = torch.cat([batch["chosen_mask"], batch["rejected_mask"]], dim=0)
        pol = seq_logprobs(policy_model, ids, mask)
        with torch.no_grad():
            ref = seq_logprobs(reference_model, ids, mask)
        return self.compute_loss(pol[:b], pol[b:], ref[:b], ref[b:])


class DPOEvaluator:
    def __init__(self, beta=0.1):
        self.beta = beta

    def _compute_dpo_loss_loader(self, dataloader, policy_model, reference_model, num_batches=None):
        """(average loss, average chosen reward, average rejected reward) as floats over the first ``num_batches`` batches of ``dataloader`` (None: all)."""
        if len(dataloader) == 0:
            return float("NaN")
        dpo_loss = DPOLoss(beta=self.beta)
        num_batches = min(num_batches, len(dataloader)) if num_batches else len(dataloader)
        totals = [0.0, 0.0, 0.0]
        for i, batch in enumerate(dataloader):
            if i >= num_batches:
                break
            for k, value in enumerate(dpo_loss.forward(batch, policy_model, reference_model)):
                totals[k] += value.item()
        return totals[0] / num_batches, totals[1] / num_batches, totals[2] / num_batches

    def evaluate(self, train_loader, val_loader, policy_model, reference_model, eval_iter=None):
        """The metrics of both loaders as a dict (``train_loss``, ``train_chosen_reward``, ``train_rejected_reward`` and the same for ``val_``); the
        policy is put in eval mode for the measurement and back in train mode after it."""
        policy_model.eval()
        with torch.no_grad():  # upstream: inference_mode; the models here keep lazily built device buffers, which must stay usable by the next training step
            train = self._compute_dpo_loss_loader(train_loader, policy_model, reference_model, num_batches=eval_iter)
            val = self._compute_dpo_loss_loader(val_loader, policy_model, reference_model, num_batches=eval_iter)
        res = {}
        for prefix, (loss, chosen, rejected) in (("train", train), ("val", val)):
            res[f"{prefix}_loss"], res[f"{prefix}_chosen_reward"], res[f"{prefix}_rejected_reward"] = loss, chosen, rejected
        policy_model.train()
        return res


def dpo_training_eval_loop_simple(
    train_loader,
    val_loader,
    policy_model,
    reference_model,
    optimizer,
    num_epoch,
    eval_freq,
    eval_iter,
    device,  # unused: the collate function puts the batch on the device
    beta=0.1,
):
    """Train ``policy_model`` with DPO against ``reference_model``; every ``eval_freq`` steps both loaders are evaluated on ``eval_iter`` batches.  Returns
    the tracked metrics as a dict of lists."""
    step = 0
    keys = ("train_losses", "val_losses", "train_chosen_rewards", "train_rejected_rewards", "val_chosen_rewards", "val_rejected_rewards")
    tracking = {k: [] for k in keys}
    dpo_loss = DPOLoss(beta=beta)
    dpo_evaluator = DPOEvaluator(beta=beta)
    for epoch in range(1, num_epoch + 1):
        policy_model.train()
        for batch in train_loader:
            step += 1
            optimizer.zero_grad()
            loss, chosen_rewards, rejected_rewards = dpo_loss.forward(batch, policy_model, reference_model)
            loss.backward()
            optimizer.step()
            if step % eval_freq == 0:
                res = dpo_evaluator.evaluate(train_loader, val_loader, policy_model, reference_model, eval_iter)
                for k in keys:  # "train_losses" <- "train_loss", "val_chosen_rewards" <- "val_chosen_reward"
                    tracking[k].append(res[k[:-2] if k.endswith("losses") else k[:-1]])
                print(
                    f"Epoch: {epoch}, Step: {step}",
                    f"Train loss: {res['train_loss']:.5f}, Val loss: {res['val_loss']:.5f}",
                    f"Train chosen reward: {res['train_chosen_reward']:.5f}",
                    f"Val chosen reward: {res['val_chosen_reward']:.5f}",
                )
    return tracking
