"""Tensor-level launchers of the Llama 3.2 / QK-Clip kernels (csrc/llama3.hip); no autograd here.

Written like ``kernels_g3.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU, allocates its
outputs with torch and enqueues on torch's current stream.  There is no CPU fallback and no launcher reads a result back to the host.
"""

import torch

from . import _lib as L

BF16, F32 = torch.bfloat16, torch.float32
HEAD_DIMS = (64, 128)
CLIP_MODES = {"per_head": 0, "naive": 1, "magnitude": 2}


def _check_heads(name, Hq, Hkv, D):
    if D not in HEAD_DIMS:
        raise ValueError(f"{name}: head_dim {D} not built {HEAD_DIMS}")
    if Hq <= 0 or Hkv <= 0 or Hq % Hkv:
        raise ValueError(f"{name}: query heads ({Hq}) must be a multiple of kv heads ({Hkv})")


def _rows(t, name, tokens, width):
    """bf16 [tokens, >= width] with unit inner stride, a row pitch that is a multiple of 8 and a 16-byte aligned base."""
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != tokens or t.shape[1] < width:
        raise ValueError(f"{name} must be bf16 [tokens={tokens}, >= {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if tokens > 1 and (t.stride(0) < width or t.stride(0) % 8):
        raise ValueError(f"{name}: row stride {t.stride(0)} must be a multiple of 8 and at least {width}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")


def _ld(t, width):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), width)


def _check_tables(name, cos, sin, pos, tokens, D):
    for t, n in ((cos, "cos"), (sin, "sin")):
        if t.dtype != F32 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] != D or t.shape[0] < 1:
            raise ValueError(f"{name}: {n} must be contiguous fp32 [rows, {D}], got {t.dtype} {tuple(t.shape)}")
    if cos.shape != sin.shape:
        raise ValueError(f"{name}: cos {tuple(cos.shape)} and sin {tuple(sin.shape)} differ")
    if pos.dtype != torch.int32 or pos.numel() != tokens or not pos.is_contiguous():
        raise ValueError(f"{name}: pos must be contiguous int32 [{tokens}]")


def rope_fwd(qkv, cos, sin, pos, Hq, Hkv, D):
    """qkv bf16 [M, (Hq + 2 Hkv) * D] (row-strided views allowed) -> (q [M, Hq * D], k [M, Hkv * D]): RoPE of the q and k heads at the positions
    ``pos`` (int32 [M]), bit for bit ``kernels.rope_apply`` on each of them."""
    L.require_gpu(qkv, cos, sin, pos)
    _check_heads("llama rope_fwd", Hq, Hkv, D)
    M = qkv.shape[0] if qkv.dim() == 2 else -1
    _rows(qkv, "llama rope_fwd: qkv", M, (Hq + 2 * Hkv) * D)
    _check_tables("llama rope_fwd", cos, sin, pos, M, D)
    q = torch.empty((M, Hq * D), dtype=BF16, device=qkv.device)
    k = torch.empty((M, Hkv * D), dtype=BF16, device=qkv.device)
    L.call("mi355_llama_rope_fwd", M, Hq, Hkv, D, L.ptr(qkv), _ld(qkv, (Hq + 2 * Hkv) * D), L.ptr(cos), L.ptr(sin), cos.shape[0], L.ptr(pos), L.ptr(q), L.ptr(k))
    return q, k


def rope_bwd(dq, dk, cos, sin, pos, dqkv, Hq, Hkv, D):
    """The adjoint rotation of dq [M, Hq * D], dk [M, Hkv * D] into the q | k columns of ``dqkv`` [M, >= (Hq + Hkv) * D] (the v columns are the
    caller's).  Returns dqkv."""
    L.require_gpu(dq, dk, cos, sin, pos, dqkv)
    _check_heads("llama rope_bwd", Hq, Hkv, D)
    M = dq.shape[0] if dq.dim() == 2 else -1
    _rows(dq, "llama rope_bwd: dq", M, Hq * D)
    _rows(dk, "llama rope_bwd: dk", M, Hkv * D)
    _rows(dqkv, "llama rope_bwd: dqkv", M, (Hq + Hkv) * D)
    _check_tables("llama rope_bwd", cos, sin, pos, M, D)
    L.call("mi355_llama_rope_bwd", M, Hq, Hkv, D, L.ptr(dq), _ld(dq, Hq * D), L.ptr(dk), _ld(dk, Hkv * D), L.ptr(cos), L.ptr(sin), cos.shape[0], L.ptr(pos),
           L.ptr(dqkv), _ld(dqkv, (Hq + Hkv) * D))
    return dqkv


def attn_max_logit(q, k, B, S, Hq, Hkv, D, key_mask=None, scale=None, out=None):
    """The largest attention logit of every query head over the batch, fp32 [Hq] on the device:
    ``max over b, j <= i, key_mask[b, j] != 0 of scale * <q[b,i,h], k[b,j,h // (Hq // Hkv)]>``.  Operands as ``kernels.attn_fwd`` takes them.
    -inf for a head without a visible pair, NaN if a visible logit is NaN."""
    L.require_gpu(q, k, key_mask, out)
    _check_heads("attn_max_logit", Hq, Hkv, D)
    if B < 0 or S < 0:
        raise ValueError(f"attn_max_logit: negative batch or sequence length ({B}, {S})")
    _rows(q, "attn_max_logit: q", B * S, Hq * D)
    _rows(k, "attn_max_logit: k", B * S, Hkv * D)
    if q.shape[1] != Hq * D or k.shape[1] != Hkv * D:
        raise ValueError(f"attn_max_logit: q / k must be [tokens, {Hq * D}] / [tokens, {Hkv * D}], got {tuple(q.shape)} / {tuple(k.shape)}")
    if key_mask is not None and not (key_mask.dtype == torch.uint8 and key_mask.is_contiguous() and tuple(key_mask.shape) == (B, S)):
        raise ValueError("attn_max_logit: key_mask must be contiguous uint8 [B, S]")
    if out is None:
        out = torch.empty(Hq, dtype=F32, device=q.device)
    elif out.dtype != F32 or not out.is_contiguous() or out.numel() != Hq:
        raise ValueError(f"attn_max_logit: out must be contiguous fp32 [{Hq}]")
    n = L.load().mi355_attn_max_logit_partials(B, S, Hq)
    part = torch.empty(max(n, 1), dtype=F32, device=q.device)
    scale = D ** -0.5 if scale is None else scale
    L.call("mi355_attn_max_logit", B, S, Hq, Hkv, D, L.ptr(q), _ld(q, Hq * D), L.ptr(k), _ld(k, Hkv * D), L.ptr(key_mask), scale, L.ptr(part), part.numel(), L.ptr(out))
    return out


def qk_clip_(wq, wk, max_logits, Hq, Hkv, tau, alpha=0.5, mode="per_head"):
    """QK-Clip of one layer in place: wq bf16 [Hq * D, d_in], wk bf16 [Hkv * D, d_in], both contiguous (arena views are); ``max_logits`` fp32 [Hq]
    on the device.  Heads that do not clip are not written; nothing is read back."""
    L.require_gpu(wq, wk, max_logits)
    if mode not in CLIP_MODES:
        raise ValueError(f"qk_clip: mode {mode!r} not one of {sorted(CLIP_MODES)}")
    for t, n, heads in ((wq, "w_queries", Hq), (wk, "w_keys", Hkv)):
        if t.dtype != BF16 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"qk_clip: {n} must be a contiguous bf16 matrix, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
        if heads <= 0 or t.shape[0] % heads:
            raise ValueError(f"qk_clip: {n} has {t.shape[0]} rows, no multiple of its {heads} heads")
    if Hq % Hkv:
        raise ValueError(f"qk_clip: query heads ({Hq}) must be a multiple of kv heads ({Hkv})")
    D, d_in = wq.shape[0] // Hq, wq.shape[1]
    if wk.shape[0] // Hkv != D or wk.shape[1] != d_in:
        raise ValueError(f"qk_clip: w_keys {tuple(wk.shape)} does not match head_dim {D} and d_in {d_in} of w_queries")
    if mode == "magnitude" and Hq != Hkv:
        raise ValueError("qk_clip: the magnitude mode is defined for multi-head attention only (num_heads == num_kv_groups)")
    if max_logits.dtype != F32 or not max_logits.is_contiguous() or max_logits.numel() != Hq:
        raise ValueError(f"qk_clip: max_logits must be contiguous fp32 [{Hq}], got {max_logits.dtype} {tuple(max_logits.shape)}")
    if not (tau > 0 and 0.0 <= alpha <= 1.0):
        raise ValueError(f"qk_clip: clip_threshold must be positive and alpha in [0, 1], got {tau}, {alpha}")
    L.call("mi355_qk_clip", Hq, Hkv, D, d_in, L.ptr(wq), L.ptr(wk), L.ptr(max_logits), float(tau), float(alpha), CLIP_MODES[mode])
