"""Tensor-level launchers of the preference-tuning kernels (csrc/preference.hip): the masked sequence average of ``DPOLoss.compute_logprobs`` over fp32
log-probs and its backward, the DPO loss of a batch (loss, reward means and both policy gradients from one launch), and the reward pooling of
``PrefRewardCalculator`` with the head's ``Linear(emb, 1)`` folded in, in four modes, forward and backward; no autograd here.

Every launcher checks shapes / dtypes on the host first (so a refusal reads the same with or without a GPU), then that the operands live on the device --
there is no CPU fallback -- and enqueues on torch's current stream.  Log-probs are fp32 ``[B, T]``; an attention mask is ``[B, T + 1]``, a reward mask ``[B, S]``,
holding 0 or 1 in bool, an integer type or a float type; hidden states are bf16 or fp32 ``[B, S, emb]``, the head's parameters bf16 or fp32 independently.
"""

import torch

from . import _lib as L
from .kernels_grpo import _MASK_CODES

BF16, F32 = torch.bfloat16, torch.float32
MODES = {"scores_mean": 0, "hidden_mean": 1, "last_token": 2, "scores_from_hidden": 3}
MAX_EMB = 8192


def _contig(t):
    return t if t.is_contiguous() else t.contiguous()


def mask_operand(mask, shape, name):
    """(tensor, dtype code) of a 0 / 1 mask of ``shape``: bool / uint8 / int32 / int64 / fp32 / bf16 are read as they are, any other integer or float
    type is cast to fp32 first."""
    if tuple(mask.shape) != tuple(shape):
        raise ValueError(f"preference: shapes disagree: {name} must be {tuple(shape)}, got {tuple(mask.shape)}")
    if mask.dtype not in _MASK_CODES:
        if mask.dtype.is_complex:
            raise TypeError(f"preference: {name} must be bool, an integer type or a float type, got {mask.dtype}")
        mask = mask.to(F32)
    return _contig(mask), _MASK_CODES[mask.dtype]


def _logp2d(logp, name="logprobs"):
    if logp.dtype != F32 or logp.dim() != 2:
        raise ValueError(f"preference: {name} must be fp32 [B, T], got {logp.dtype} {tuple(logp.shape)}")
    if logp.shape[0] < 1 or logp.shape[1] < 1:
        raise ValueError(f"preference: empty {name} {tuple(logp.shape)}")
    return _contig(logp)


def seq_logprob_fwd(logp, mask=None):
    """(avg, den), fp32 [B]: avg[b] = sum_t logp[b, t] mask[b, t + 1] / sum_s mask[b, s] with ``mask`` the unshifted attention mask [B, T + 1] (an all-zero
    mask: NaN); without a mask the mean over the T labels."""
    logp = _logp2d(logp)
    B, T = logp.shape
    mdt = 0
    if mask is not None:
        mask, mdt = mask_operand(mask, (B, T + 1), "attention_mask")
    L.require_gpu(logp, mask)
    avg = torch.empty((B,), dtype=F32, device=logp.device)
    den = torch.empty((B,), dtype=F32, device=logp.device)
    L.call("mi355_dpo_seq_logprob", B, T, L.ptr(logp), L.ptr(mask), mdt, L.ptr(avg), L.ptr(den))
    return avg, den


def _vec(t, name, n):
    if t.dtype != F32 or t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"preference: shapes disagree: {name} must be fp32 [{n}], got {t.dtype} {tuple(t.shape)}")
    return _contig(t)


def seq_logprob_bwd(g, mask, den, T):
    """dlogp fp32 [B, T] = g[b] mask[b, t + 1] / den[b]."""
    B = den.shape[0]
    g, den = _vec(g, "gradient", B), _vec(den, "den", B)
    mdt = 0
    if mask is not None:
        mask, mdt = mask_operand(mask, (B, T + 1), "attention_mask")
    L.require_gpu(g, den, mask)
    dlogp = torch.empty((B, T), dtype=F32, device=g.device)
    L.call("mi355_dpo_seq_logprob_bwd", B, T, L.ptr(g), L.ptr(mask), mdt, L.ptr(den), L.ptr(dlogp))
    return dlogp


def dpo_loss(pol_chosen, pol_rejected, ref_chosen, ref_rejected, beta, label_smoothing, want_grad=True):
    """(out fp32 [3] = loss, mean chosen reward, mean rejected reward; d loss / d pol_chosen; d loss / d pol_rejected), the gradients fp32 [b] or None."""
    if pol_chosen.dim() != 1 or pol_chosen.shape[0] < 1:
        raise ValueError(f"preference: the DPO loss takes four fp32 [b] vectors of log-probs, got {tuple(pol_chosen.shape)}")
    n = pol_chosen.shape[0]
    pc, pr = _vec(pol_chosen, "pol_chosen_logprob", n), _vec(pol_rejected, "pol_rejected_logprob", n)
    rc, rr = _vec(ref_chosen, "ref_chosen_logprob", n), _vec(ref_rejected, "ref_rejected_logprob", n)
    L.require_gpu(pc, pr, rc, rr)
    out = torch.empty((3,), dtype=F32, device=pc.device)
    dpc = torch.empty((n,), dtype=F32, device=pc.device) if want_grad else None
    dpr = torch.empty((n,), dtype=F32, device=pc.device) if want_grad else None
    L.call("mi355_dpo_loss", n, L.ptr(pc), L.ptr(pr), L.ptr(rc), L.ptr(rr), float(beta), float(label_smoothing), L.ptr(out), L.ptr(dpc), L.ptr(dpr))
    return out, dpc, dpr


def check_head(weight, bias, E):
    """The head's parameters as the kernels read them: (w [E] contiguous, bias [1] or None), bf16 or fp32, both of one dtype."""
    if weight.dtype not in (BF16, F32):
        raise TypeError(f"preference: the head's weight must be bf16 or fp32, got {weight.dtype}")
    if weight.numel() != E or weight.dim() > 2 or (weight.dim() == 2 and weight.shape[0] != 1):
        raise ValueError(f"preference: shapes disagree: model_head must be a Linear({E}, 1), its weight is {tuple(weight.shape)}")
    if bias is not None and (bias.numel() != 1 or bias.dtype != weight.dtype):
        raise ValueError(f"preference: the head's bias must hold one {weight.dtype} value, got {bias.dtype} {tuple(bias.shape)}")
    return _contig(weight).view(E), (None if bias is None else bias.reshape(1))


def check_hidden(hidden, mask, mode, what="hidden_states"):
    """(B, S, E) of the pooled operand: hidden states bf16 / fp32 [B, S, emb] with emb a multiple of 8, at most 8 192; mode 0: the scores [B, S, 1]."""
    if hidden.dtype not in (BF16, F32):
        raise TypeError(f"preference: {what} must be bf16 or fp32, got {hidden.dtype}")
    if hidden.dim() != 3:
        raise ValueError(f"preference: {what} must be 3-D (b, s, {'1' if mode == 0 else 'emb_dim'}), got {tuple(hidden.shape)}")
    B, S, E = hidden.shape
    if B < 1 or S < 1:
        raise ValueError(f"preference: empty {what} {tuple(hidden.shape)}")
    if mode == 0:
        if E != 1:
            raise ValueError(f"preference: rewards must be the head's output (b, s, 1), got {tuple(hidden.shape)}")
    elif E % 8 or E < 8 or E > MAX_EMB:
        raise ValueError(f"preference: emb_dim must be a multiple of 8, at most {MAX_EMB}, got {E}")
    return B, S, E


def reward_pool_fwd(mode, hidden, mask, weight=None, bias=None):
    """(score fp32 [B], pooled fp32 [B, E] or None, count fp32 [B]) of one of ``MODES`` (include/mi355_vlm.h); ``weight`` [E], ``bias`` [1] or None."""
    B, S, E = check_hidden(hidden, mask, mode)
    mask, mdt = mask_operand(mask, (B, S), "the mask")
    hidden = _contig(hidden)
    L.require_gpu(hidden, mask, weight, bias)
    dev = hidden.device
    score = torch.empty((B,), dtype=F32, device=dev)
    count = torch.empty((B,), dtype=F32, device=dev)
    pooled = None if mode == 0 else torch.empty((B, E), dtype=F32, device=dev)
    L.call("mi355_reward_pool_fwd", mode, B, S, E, L.ptr(hidden), L.dt_code(hidden.dtype), L.ptr(mask), mdt, L.ptr(weight),
           0 if weight is None else L.dt_code(weight.dtype), L.ptr(bias), L.ptr(score), L.ptr(pooled), L.ptr(count))
    return score, pooled, count


def reward_pool_bwd(mode, g, shape, hidden_dtype, mask, count, weight=None, pooled=None, want_dx=True, want_dw=True, want_dbias=True):
    """(dx in ``hidden_dtype`` of ``shape`` with exact zeros on the rows the forward skipped, dw [E], dbias [1]) -- None where not wanted."""
    B, S, E = shape
    g, count = _vec(g, "gradient", B), _vec(count, "count", B)
    mask, mdt = mask_operand(mask, (B, S), "the mask")
    L.require_gpu(g, count, mask, weight, pooled)
    dev = g.device
    want_dw, want_dbias = want_dw and mode != 0, want_dbias and mode != 0
    dx = torch.empty(shape, dtype=hidden_dtype, device=dev) if want_dx else None
    dw = torch.empty((E,), dtype=weight.dtype, device=dev) if want_dw else None
    db = torch.empty((1,), dtype=weight.dtype, device=dev) if want_dbias else None
    if dx is None and dw is None and db is None:
        return None, None, None
    L.call("mi355_reward_pool_bwd", mode, B, S, E, L.ptr(g), L.ptr(mask), mdt, L.ptr(count), L.ptr(weight), 0 if weight is None else L.dt_code(weight.dtype),
           L.ptr(pooled), L.ptr(dx), L.dt_code(hidden_dtype), L.ptr(dw), L.ptr(db))
    return dx, dw, db
