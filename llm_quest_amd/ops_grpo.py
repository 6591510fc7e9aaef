"""Autograd nodes of the GRPO loss layer on the launchers of ``kernels_grpo.py`` / ``kernels_grpo_head.py``: the label log-probs over the logits, the
same from the hidden states on a vocabulary-chunked LM head, the per-token chain as one node, the one-pass logits loss, and one small node per
reference-named per-token function.  The kernels write the gradients; a node's backward hands
them on, times the incoming gradient where that is not known to be one."""

import torch

from . import kernels as K0
from . import kernels_grpo as K
from . import kernels_grpo_head as KH
from .ops import arena_for

F32 = torch.float32


def _times(grad, g):
    """``grad`` (fp32, stored by a forward) times the incoming scalar gradient ``g``, on the device."""
    return K.scale(grad, g)


def _scale_logits_grad(dl, g):
    """bf16 d loss / d logits times the incoming gradient.  ``loss.backward()`` passes exactly 1: that is read once on the host and the pass over the
    logits (as large as the loss pass itself) is skipped."""
    if float(g) == 1.0:
        return dl
    flat = dl if dl.is_contiguous() else dl.contiguous()
    return K0.scale_bf16(flat, g.to(F32).reshape(1), out=flat).view(dl.shape)


class LabelLogProbFn(torch.autograd.Function):
    """``log_probs_per_token``: fp32 [B, S - 1] from bf16 logits [B, S, V] and int64 ids [B, S].  Backward: ``label_logprob_bwd`` into a fresh buffer (the
    logits belong to the caller), or with ``inplace`` into the logits themselves, which are then consumed."""

    @staticmethod
    def forward(ctx, logits, ids, inplace):
        logp, lse = K.label_logprob_fwd(logits, ids)
        ctx.saved = (logits, ids, lse)
        ctx.inplace = inplace
        return logp

    @staticmethod
    def backward(ctx, g):
        logits, ids, lse = ctx.saved
        ctx.saved = None
        g = g.to(F32)
        dl = K.label_logprob_bwd(g if g.is_contiguous() else g.contiguous(), logits, lse, ids, out=logits if ctx.inplace else None)
        return dl.detach(), None, None


class HeadLogProbFn(torch.autograd.Function):
    """``log_probs_per_token_from_hidden``: fp32 [B, S - 1] from bf16 hidden states [B, S, D], int64 ids [B, S] and the (possibly tied) head weight of
    ``owner``, chunk by chunk; the logits are never held.  Backward walks the chunks again: dh comes back, the weight's gradient goes to the owner's
    arena (accumulating where the embedding's backward shares it).  The incoming gradient is a weight per token and is multiplied in by the kernel."""

    @staticmethod
    def forward(ctx, hidden, ids, owner, weight, vocab_chunk):
        arena_for(owner)
        logp, lse = KH.head_logprob_fwd(hidden, weight, ids, vocab_chunk)
        ctx.saved = (hidden, ids, lse)
        ctx.owner, ctx.weight, ctx.vocab_chunk = owner, weight, vocab_chunk
        return logp

    @staticmethod
    def backward(ctx, g):
        hidden, ids, lse = ctx.saved
        ctx.saved = None
        w = ctx.weight
        view, acc = arena_for(ctx.owner).grad_target(w) if w.requires_grad else (None, False)
        g = g.to(F32)
        dh = KH.head_logprob_bwd(g if g.is_contiguous() else g.contiguous(), hidden, w, lse, ids, ctx.vocab_chunk, dw_out=view, dw_accumulate=acc)
        return dh, None, None, None, None


class TokenLossFn(torch.autograd.Function):
    """The whole per-token chain from the policy's log-probs: one kernel gives the loss and d loss / d policy_logp."""

    @staticmethod
    def forward(ctx, policy_logp, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen, variant, unbiased_kl, delta):
        loss, dlogp, opm, mean_kl = K.token_loss(policy_logp, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen,
                                                 variant, unbiased_kl, delta, want_grad=True)
        ctx.dlogp = dlogp
        ctx.mark_non_differentiable(opm, mean_kl)
        return loss.clone(), opm, mean_kl

    @staticmethod
    def backward(ctx, g, _gm, _gk):
        return (_times(ctx.dlogp, g),) + (None,) * 12


class LogitsLossFn(torch.autograd.Function):
    """The one-pass path: loss and d loss / d logits from one read of each logits row.  With ``inplace`` the gradient overwrites the logits."""

    @staticmethod
    def forward(ctx, logits, ids, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen, variant, unbiased_kl, inplace):
        loss, terms, logp, dl = K.logits_loss(logits, ids, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen,
                                              variant, unbiased_kl, out=logits if inplace else None)
        ctx.dl = dl
        ctx.mark_non_differentiable(logp)
        return loss.clone(), logp

    @staticmethod
    def backward(ctx, g, _gl):
        dl, ctx.dl = ctx.dl, None
        if dl is None:
            raise RuntimeError("grpo_policy_loss: the logits' gradient was already handed on (a second backward through the one-pass node)")
        return (_scale_logits_grad(dl.detach(), g),) + (None,) * 13


# ------------------------------------------------------------------------------------------------ the reference-named pieces
class KlDivFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pol, ref, ratio):
        shape = tuple(pol.shape)
        pol, ref = K.tok2d(pol, "policy_logprobs"), K.tok2d(ref, "reference_logprobs", shape)
        ratio = None if ratio is None else K.tok2d(ratio, "policy_ratio", shape)
        ctx.saved = (pol, ref, ratio)
        return K.piece(K.OP_KL_FWD, shape[0], shape[1], pol, ref, ratio, outs=(shape, None, None))[0]

    @staticmethod
    def backward(ctx, g):
        pol, ref, ratio = ctx.saved
        shape = tuple(pol.shape)
        dp, dr, drho = K.piece(K.OP_KL_BWD, shape[0], shape[1], pol, ref, ratio, K.tok2d(g, "gradient", shape),
                               outs=(shape, shape, None if ratio is None else shape))
        return dp, dr, drho


class SurrogateFn(torch.autograd.Function):
    """The clipped (p0 = min_clip, p1 = max_clip) or, with ``sapo``, the soft-gate surrogate (p0 / p1 = the temperatures); advantages carry no gradient."""

    @staticmethod
    def forward(ctx, ratio, advantages, p0, p1, sapo):
        ratio = K.tok2d(ratio, "policy_ratio")
        B, T = ratio.shape
        adv = K.seq1d(advantages, "advantages_broadcast", B)
        ctx.saved, ctx.args = (ratio, adv), (p0, p1, int(sapo))
        return K.piece(K.OP_SURR_FWD, B, T, ratio, adv, p=(p0, p1, 0.0), flag=int(sapo), outs=((B, T), None, None))[0]

    @staticmethod
    def backward(ctx, g):
        ratio, adv = ctx.saved
        B, T = ratio.shape
        p0, p1, sapo = ctx.args
        dr = K.piece(K.OP_SURR_BWD, B, T, ratio, adv, x3=K.tok2d(g, "gradient", (B, T)), p=(p0, p1, 0.0), flag=sapo, outs=((B, T), None, None))[0]
        return dr, None, None, None, None


class SeqMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logp, loss_mask):
        logp = K.tok2d(logp, "logprobs_per_token")
        B, T = logp.shape
        ctx.saved = (loss_mask, B, T)
        return K.piece(K.OP_SEQ_MEAN_FWD, B, T, logp, mask=loss_mask, outs=((B,), None, None))[0]

    @staticmethod
    def backward(ctx, g):
        loss_mask, B, T = ctx.saved
        g = K.seq1d(g, "gradient", B)
        return K.piece(K.OP_SEQ_MEAN_BWD, B, T, g, x3=g, mask=loss_mask, outs=((B, T), None, None))[0], None


class RatioLossFn(torch.autograd.Function):
    """``GRPOLoss.compute`` for the token-level variants: the loss from (ratio, kl), with d loss / d ratio and d loss / d kl from the same kernel."""

    @staticmethod
    def forward(ctx, ratio, kl, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen, variant, off_policy_mask):
        ratio = K.tok2d(ratio, "policy_ratio")
        B, T = ratio.shape
        kl = K.tok2d(kl, "kl_div", (B, T))
        adv = K.seq1d(advantages, "advantages", B)
        opm = None if off_policy_mask is None else K.seq1d(off_policy_mask, "off_policy_mask", B)
        code = K.check_scalars(B, num_samples, max_gen, variant)
        y0, dr, dk = K.piece(K.OP_RATIO_LOSS, B, T, ratio, adv, kl, opm, mask=loss_mask, p=(min_clip, max_clip, beta), flag=code, num_samples=num_samples,
                             max_gen=max_gen, outs=((1,), (B, T), (B, T)))
        ctx.grads = (dr, dk)
        return y0[0].clone()

    @staticmethod
    def backward(ctx, g):
        dr, dk = ctx.grads
        return (_times(dr, g), _times(dk, g)) + (None,) * 9


class GspoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ratio, advantages, min_clip, max_clip, off_policy_mask):
        if ratio.dtype != F32 or ratio.dim() != 1:
            raise ValueError(f"grpo: gspo takes the sequence-level ratio, fp32 [B], got {ratio.dtype} {tuple(ratio.shape)}")
        B = ratio.shape[0]
        adv = K.seq1d(advantages, "advantages", B)
        opm = None if off_policy_mask is None else K.seq1d(off_policy_mask, "off_policy_mask", B)
        y0, dr, _ = K.piece(K.OP_GSPO_LOSS, 1, B, ratio.contiguous(), adv, x3=opm, p=(min_clip, max_clip, 0.0), outs=((1,), (B,), None))
        ctx.dr = dr
        return y0[0].clone()

    @staticmethod
    def backward(ctx, g):
        return (_times(ctx.dr, g),) + (None,) * 4


class AggregateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loss_per_token, loss_mask, num_samples, max_gen, variant):
        x = K.tok2d(loss_per_token, "loss_per_token")
        B, T = x.shape
        code = K.check_scalars(B, num_samples, max_gen, variant)
        y0, dx, _ = K.piece(K.OP_AGGREGATE, B, T, x, mask=loss_mask, flag=code, num_samples=num_samples, max_gen=max_gen, outs=((1,), (B, T), None))
        ctx.dx = dx
        return y0[0].clone()

    @staticmethod
    def backward(ctx, g):
        return (_times(ctx.dx, g),) + (None,) * 4


def off_policy(kl, advantages, loss_mask, delta):
    """(mean_kl fp32 [B], mask bool [B, 1]); no gradient."""
    kl = K.tok2d(kl.detach(), "kl_div_per_token")
    B, T = kl.shape
    mean, m, _ = K.piece(K.OP_OFF_POLICY, B, T, kl, K.seq1d(advantages.detach(), "advantages", B), mask=loss_mask, p=(delta, 0.0, 0.0), outs=((B,), (B,), None))
    return mean, (m != 0).view(B, 1)
