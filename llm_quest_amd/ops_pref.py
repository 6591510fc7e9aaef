"""Autograd nodes of preference tuning on the launchers of ``kernels_pref.py``: the masked sequence average of the label log-probs (its gradient is the weight
per token that ``ops_grpo.LabelLogProbFn`` / ``HeadLogProbFn`` take unchanged), the DPO loss as one node, and the reward pooling with the head folded in.  The
kernels write the gradients; a node's backward hands them on, times the incoming gradient where a forward already stored them."""

import torch

from . import kernels_grpo as KG
from . import kernels_pref as K

F32 = torch.float32


class SeqLogProbFn(torch.autograd.Function):
    """``DPOLoss.compute_logprobs`` after the gather: fp32 [B] from fp32 log-probs [B, T] and the unshifted attention mask [B, T + 1] (or None)."""

    @staticmethod
    def forward(ctx, logp, mask):
        avg, den = K.seq_logprob_fwd(logp, mask)
        ctx.saved = (mask, den, logp.shape[1])
        return avg

    @staticmethod
    def backward(ctx, g):
        mask, den, T = ctx.saved
        g = g.to(F32)
        return K.seq_logprob_bwd(g if g.is_contiguous() else g.contiguous(), mask, den, T), None


class DpoLossFn(torch.autograd.Function):
    """``DPOLoss.compute_loss``: (loss, mean chosen reward, mean rejected reward), all 0-d fp32, from one launch that also writes d loss / d pol_chosen
    and d loss / d pol_rejected.  The rewards are detached, as upstream; the reference policy's log-probs carry no gradient."""

    @staticmethod
    def forward(ctx, pol_chosen, pol_rejected, ref_chosen, ref_rejected, beta, label_smoothing):
        out, dpc, dpr = K.dpo_loss(pol_chosen, pol_rejected, ref_chosen, ref_rejected, beta, label_smoothing, want_grad=True)
        ctx.grads = (dpc, dpr)
        loss, chosen, rejected = out[0].clone(), out[1], out[2]
        ctx.mark_non_differentiable(chosen, rejected)
        return loss, chosen, rejected

    @staticmethod
    def backward(ctx, g, _gc, _gr):
        dpc, dpr = ctx.grads
        return KG.scale(dpc, g), KG.scale(dpr, g), None, None, None, None


class RewardPoolFn(torch.autograd.Function):
    """One mode of ``kernels_pref.MODES``: fp32 [B] scores from (hidden states or scores, mask, the head's weight and bias)."""

    @staticmethod
    def forward(ctx, hidden, mask, weight, bias, mode):
        w, b = (None, None) if mode == 0 else K.check_head(weight, bias, hidden.shape[2])
        score, pooled, count = K.reward_pool_fwd(mode, hidden, mask, w, b)
        ctx.saved = (mask, w, pooled, count)
        ctx.meta = (mode, tuple(hidden.shape), hidden.dtype, None if weight is None else tuple(weight.shape), None if bias is None else tuple(bias.shape))
        return score

    @staticmethod
    def backward(ctx, g):
        mask, w, pooled, count = ctx.saved
        mode, shape, hdt, wshape, bshape = ctx.meta
        g = g.to(F32)
        need = ctx.needs_input_grad
        dx, dw, db = K.reward_pool_bwd(mode, g if g.is_contiguous() else g.contiguous(), shape, hdt, mask, count, w, pooled, want_dx=need[0],
                                       want_dw=need[2], want_dbias=need[3] and bshape is not None)
        return dx, None, (None if dw is None else dw.view(wshape)), (None if db is None else db.view(bshape)), None
