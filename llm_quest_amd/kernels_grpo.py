"""Tensor-level launchers of the GRPO kernels (csrc/grpo.hip): the label log-probs over bf16 logits and their backward, the per-token loss chain
of the five variants, the one-pass logits loss, and the small per-token pieces behind the reference-named functions; no autograd here.

Every launcher checks shapes / strides / dtypes on the host first (so a refusal reads the same with or without a GPU), then that the operands live
on the device -- there is no CPU fallback -- and enqueues on torch's current stream.  Logits are bf16 ``[B, S, V]`` views whose last dimension is
contiguous and whose batch stride and row pitch are multiples of 8 elements (``rows_are_vector_ready`` says whether a padded copy is needed); ids are int64
``[B, S]``; the per-token operands are fp32 ``[B, T]`` with ``T = S - 1``; ``loss_mask`` holds 0 or 1 in bool, an integer type or a float type.
"""

import torch

from . import _lib as L

BF16, F32, I64, U8 = torch.bfloat16, torch.float32, torch.int64, torch.uint8
VARIANTS = {"grpo": 0, "dapo": 1, "dr_grpo": 2, "sapo": 3, "gspo": 4}
_MASK_CODES = {torch.bool: 0, torch.uint8: 0, torch.int32: 1, torch.int64: 2, torch.float32: 3, torch.bfloat16: 4}


def variant_code(variant):
    if variant not in VARIANTS:
        raise ValueError(f"Unknown loss type: {variant}")
    return VARIANTS[variant]


def rows_are_vector_ready(logits):
    """True when the kernels can address ``logits`` [B, S, V] as it stands: unit stride in V, batch stride and row pitch multiples of 8 elements,
    rows that do not overlap, a 16-byte aligned pointer."""
    return (logits.stride(2) == 1 and logits.stride(1) % 8 == 0 and logits.stride(0) % 8 == 0 and logits.stride(1) >= logits.shape[2]
            and logits.data_ptr() % 16 == 0)


def check_logits_ids(logits, ids, what="grpo"):
    """The shape / dtype refusals shared by every function that takes (logits, inputs); returns (B, S, V)."""
    if logits.dtype != BF16:
        raise TypeError(f"{what}: the logits must be bf16 (the HIP path has no other precision), got {logits.dtype}")
    if logits.dim() != 3:
        raise ValueError(f"{what}: the logits must be 3-D (B, S, vocab_size), got {tuple(logits.shape)}")
    B, S, V = logits.shape
    if ids.dtype != I64 or ids.dim() != 2:
        raise TypeError(f"{what}: the inputs must be int64 [B, S], got {ids.dtype} {tuple(ids.shape)}")
    if tuple(ids.shape) != (B, S):
        raise ValueError(f"{what}: shapes disagree: logits {tuple(logits.shape)} against inputs {tuple(ids.shape)}")
    if B < 1 or V < 1:
        raise ValueError(f"{what}: empty logits {tuple(logits.shape)}")
    return B, S, V


def _vector_rows(logits, name):
    if not rows_are_vector_ready(logits):
        raise ValueError(f"grpo: {name} must have 16-byte rows for the vector path (unit stride in V, batch stride and row pitch multiples of 8 "
                         f"elements, 16-byte aligned): strides {tuple(logits.stride())}; pad the rows first")


def _tok(t, name, B, T):
    if t.dtype != F32 or tuple(t.shape) != (B, T):
        raise ValueError(f"grpo: shapes disagree: {name} must be fp32 {(B, T)}, got {t.dtype} {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


def _adv(a, B):
    if a.dtype != F32 or a.numel() != B:
        raise ValueError(f"grpo: shapes disagree: advantages must be fp32 with {B} values, got {a.dtype} {tuple(a.shape)}")
    return a.reshape(B).contiguous()


def mask_operand(mask, B, T):
    """(tensor, dtype code) of a loss mask [B, T]: bool / uint8 / int32 / int64 / fp32 / bf16 are read as they are, any other integer or float type is
    cast to fp32 first."""
    if tuple(mask.shape) != (B, T):
        raise ValueError(f"grpo: shapes disagree: loss_mask must be {(B, T)}, got {tuple(mask.shape)}")
    if mask.dtype not in _MASK_CODES:
        if mask.dtype.is_complex:
            raise TypeError(f"grpo: loss_mask must be bool, an integer type or a float type, got {mask.dtype}")
        mask = mask.to(F32)
    return (mask if mask.is_contiguous() else mask.contiguous()), _MASK_CODES[mask.dtype]


def check_scalars(B, num_samples, max_gen, variant):
    code = variant_code(variant)
    if int(num_samples) < 1 or int(max_gen) < 1:
        raise ValueError(f"grpo: num_samples ({num_samples}) and max_gen ({max_gen}) must be positive")
    if variant in ("grpo", "sapo") and B % int(num_samples):
        raise ValueError(f"grpo: the batch ({B}) is not divisible by num_samples ({num_samples}), which {variant} needs for its groups")
    return code


def label_logprob_fwd(logits, ids):
    """(logp, lse), both fp32 [B, S - 1]: logp[b, s] = logits[b, s, ids[b, s + 1]] - logsumexp(logits[b, s, :]).  ``S == 1``: empty results, no launch."""
    B, S, V = check_logits_ids(logits, ids, "label_logprob")
    _vector_rows(logits, "logits")
    L.require_gpu(logits, ids)
    logp = torch.empty((B, S - 1), dtype=F32, device=logits.device)
    lse = torch.empty((B, S - 1), dtype=F32, device=logits.device)
    if S > 1:
        ids = ids if ids.is_contiguous() else ids.contiguous()
        L.call("mi355_label_logprob_fwd", B, S, V, L.ptr(logits), logits.stride(0), logits.stride(1), L.ptr(ids), L.ptr(logp), L.ptr(lse))
    return logp, lse


def grad_buffer(logits):
    """A fresh bf16 [B, S, V] view on rows of a 16-byte pitch, for a gradient that must not overwrite the logits."""
    B, S, V = logits.shape
    return torch.empty((B, S, (V + 7) // 8 * 8), dtype=BF16, device=logits.device)[:, :, :V]


def label_logprob_bwd(g, logits, lse, ids, out=None):
    """dlogits bf16 [B, S, V] = g[b, s] (onehot(ids[b, s + 1]) - exp(logits - lse)), row S - 1 of every sample exact zeros.  ``out``: where to write
    (``logits`` itself: in place); None: a fresh buffer."""
    B, S, V = check_logits_ids(logits, ids, "label_logprob")
    _vector_rows(logits, "logits")
    g, lse = _tok(g, "g", B, S - 1), _tok(lse, "lse", B, S - 1)
    if out is None:
        out = grad_buffer(logits)
    if out.dtype != BF16 or tuple(out.shape) != (B, S, V):
        raise ValueError(f"grpo: shapes disagree: dlogits must be bf16 {(B, S, V)}, got {out.dtype} {tuple(out.shape)}")
    _vector_rows(out, "dlogits")
    L.require_gpu(g, logits, lse, ids, out)
    if S == 1:
        out.zero_()
        return out
    ids = ids if ids.is_contiguous() else ids.contiguous()
    L.call("mi355_label_logprob_bwd", B, S, V, L.ptr(g), L.ptr(logits), logits.stride(0), logits.stride(1), L.ptr(lse), L.ptr(ids), L.ptr(out),
           out.stride(0), out.stride(1))
    return out


def token_loss(policy_logp, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen=1, variant="grpo",
               unbiased_kl=False, delta=None, want_grad=True):
    """The per-token chain on fp32 [B, T] log-probs.  Returns (loss fp32 0-d, dlogp fp32 [B, T] or None, off_policy_mask bool [B], mean_kl fp32 [B]);
    ``delta`` None: no off-policy mask (all True)."""
    if policy_logp.dim() != 2:
        raise ValueError(f"grpo: shapes disagree: policy log-probs must be 2-D (B, T), got {tuple(policy_logp.shape)}")
    B, T = policy_logp.shape
    code = check_scalars(B, num_samples, max_gen, variant)
    pol, old, ref = _tok(policy_logp, "policy_logprobs", B, T), _tok(old_logp, "old_logprobs", B, T), _tok(ref_logp, "reference_logprobs", B, T)
    adv = _adv(advantages, B)
    mask, mdt = mask_operand(loss_mask, B, T)
    if B < 1 or T < 1:
        raise ValueError(f"grpo: empty log-probs {(B, T)}")
    L.require_gpu(pol, old, ref, adv, mask)
    dev = pol.device
    loss = torch.empty((1,), dtype=F32, device=dev)
    dlogp = torch.empty((B, T), dtype=F32, device=dev) if want_grad else None
    opm = torch.empty((B,), dtype=torch.bool, device=dev)
    mean_kl = torch.empty((B,), dtype=F32, device=dev)
    ws = torch.empty((4 * B + 2,), dtype=F32, device=dev)
    L.call("mi355_grpo_token_loss", B, T, L.ptr(pol), L.ptr(old), L.ptr(ref), L.ptr(adv), L.ptr(mask), mdt, float(min_clip), float(max_clip), float(beta),
           float(0.0 if delta is None else delta), int(num_samples), int(max_gen), code, int(bool(unbiased_kl)), int(delta is not None), L.ptr(loss),
           L.ptr(dlogp), L.ptr(opm), L.ptr(mean_kl), L.ptr(ws))
    return loss[0], dlogp, opm, mean_kl


def logits_loss(logits, ids, old_logp, ref_logp, advantages, loss_mask, min_clip, max_clip, beta, num_samples, max_gen=1, variant="grpo",
                unbiased_kl=False, use_off_policy_mask=False, out=None):
    """The one-pass path: reads each logits row once and writes d loss / d logits to ``out`` (``logits`` itself: in place; None: a fresh buffer).
    Returns (loss fp32 0-d, terms fp32 [B, T], policy_logp fp32 [B, T], dlogits).  Token-level variants without the off-policy mask only."""
    code = variant_code(variant)
    if variant == "gspo":
        raise ValueError("grpo one-pass: gspo needs each sequence's ratio before any row's weight is known; use the two-pass path")
    if use_off_policy_mask:
        raise ValueError("grpo one-pass: the off-policy mask needs each sequence's mean KL before any row's weight is known; use the two-pass path")
    B, S, V = check_logits_ids(logits, ids, "grpo one-pass")
    if S < 2:
        raise ValueError("grpo one-pass: the sequences need at least two positions")
    T = S - 1
    check_scalars(B, num_samples, max_gen, variant)
    _vector_rows(logits, "logits")
    old, ref = _tok(old_logp, "old_logprobs", B, T), _tok(ref_logp, "reference_logprobs", B, T)
    adv = _adv(advantages, B)
    mask, mdt = mask_operand(loss_mask, B, T)
    if out is None:
        out = grad_buffer(logits)
    if out.dtype != BF16 or tuple(out.shape) != (B, S, V):
        raise ValueError(f"grpo: shapes disagree: dlogits must be bf16 {(B, S, V)}, got {out.dtype} {tuple(out.shape)}")
    _vector_rows(out, "dlogits")
    L.require_gpu(logits, ids, old, ref, adv, mask, out)
    dev = logits.device
    ids = ids if ids.is_contiguous() else ids.contiguous()
    loss = torch.empty((1,), dtype=F32, device=dev)
    terms = torch.empty((B, T), dtype=F32, device=dev)
    logp = torch.empty((B, T), dtype=F32, device=dev)
    ws = torch.empty((4 * B + 2,), dtype=F32, device=dev)
    L.call("mi355_grpo_logits_loss", B, S, V, L.ptr(logits), logits.stride(0), logits.stride(1), L.ptr(out), out.stride(0), out.stride(1), L.ptr(ids),
           L.ptr(old), L.ptr(ref), L.ptr(adv), L.ptr(mask), mdt, float(min_clip), float(max_clip), float(beta), int(num_samples), int(max_gen), code,
           int(bool(unbiased_kl)), 0, L.ptr(loss), L.ptr(terms), L.ptr(logp), L.ptr(ws))
    return loss[0], terms, logp, out


# the ops of mi355_grpo_piece (include/mi355_vlm.h)
OP_KL_FWD, OP_KL_BWD, OP_SURR_FWD, OP_SURR_BWD, OP_SEQ_MEAN_FWD, OP_SEQ_MEAN_BWD = 1, 2, 3, 4, 5, 6
OP_RATIO_LOSS, OP_GSPO_LOSS, OP_AGGREGATE, OP_OFF_POLICY, OP_SCALE = 7, 8, 9, 10, 11


def tok2d(t, name, shape=None):
    """An fp32 2-D per-token operand, contiguous; ``shape``: what it must agree with."""
    if t.dtype != F32 or t.dim() != 2:
        raise ValueError(f"grpo: {name} must be fp32 [B, T], got {t.dtype} {tuple(t.shape)}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"grpo: shapes disagree: {name} is {tuple(t.shape)}, expected {tuple(shape)}")
    return t if t.is_contiguous() else t.contiguous()


def seq1d(t, name, B):
    """An fp32 per-sequence operand ([B], [B, 1] or [1, B]), as a contiguous [B] (bool masks are cast)."""
    if t.numel() != B:
        raise ValueError(f"grpo: shapes disagree: {name} must hold {B} values, got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(F32)
    if t.dtype != F32:
        raise ValueError(f"grpo: {name} must be fp32, got {t.dtype}")
    return t.reshape(B).contiguous()


def piece(op, B, T, x0, x1=None, x2=None, x3=None, mask=None, p=(0.0, 0.0, 0.0), flag=0, num_samples=1, max_gen=1, outs=((), None, None)):
    """One op of ``mi355_grpo_piece``; ``outs``: the shapes of y0 / y1 / y2 (None: not written).  Operands are already checked by the caller."""
    mdt = 0
    if mask is not None:
        mask, mdt = mask_operand(mask, B, T)
    L.require_gpu(x0, x1, x2, x3, mask)
    ys = [None if s is None else torch.empty(s, dtype=F32, device=x0.device) for s in outs]
    ws = torch.empty((4 * B + 2,), dtype=F32, device=x0.device) if op in (OP_RATIO_LOSS, OP_AGGREGATE) else None
    L.call("mi355_grpo_piece", op, B, T, L.ptr(x0), L.ptr(x1), L.ptr(x2), L.ptr(x3), L.ptr(mask), mdt, float(p[0]), float(p[1]), float(p[2]), int(flag),
           int(num_samples), int(max_gen), L.ptr(ys[0]), L.ptr(ys[1]), L.ptr(ys[2]), L.ptr(ws))
    return ys


def scale(x, g):
    """x * g for an fp32 tensor and a one-element fp32 device tensor (a stored gradient times the incoming one)."""
    x = x if x.is_contiguous() else x.contiguous()
    g = g.to(F32).reshape(1)
    return piece(OP_SCALE, 1, x.numel(), x, x3=g, outs=(tuple(x.shape), None, None))[0]
