"""Tensor-level launchers of the Reinforced Attention Learning kernels (csrc/ral.hip); no autograd here.

Written like ``kernels_llama.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU, allocates its
outputs with torch and enqueues on torch's current stream.  There is no CPU fallback and no launcher reads a result back to the host.

``P`` / ``Q`` (the prepared, head-averaged attention distributions), ``dP`` and ``da`` are fp32 [B, S, S]; ``Z`` fp32 [B, S]; ``lse`` fp32 [B, Hq, S].
"""

import torch

from . import _lib as L
from .kernels_llama import _check_heads, _ld, _rows

BF16, F32 = torch.bfloat16, torch.float32


def _f32(t, name, shape):
    if t.dtype != F32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous fp32 {list(shape)}, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")


def _check_qk(name, q, k, B, S, Hq, Hkv, D, key_mask):
    _check_heads(name, Hq, Hkv, D)
    if B < 0 or S < 0:
        raise ValueError(f"{name}: negative batch or sequence length ({B}, {S})")
    _rows(q, f"{name}: q", B * S, Hq * D)
    _rows(k, f"{name}: k", B * S, Hkv * D)
    if q.shape[1] != Hq * D or k.shape[1] != Hkv * D:
        raise ValueError(f"{name}: q / k must be [tokens, {Hq * D}] / [tokens, {Hkv * D}], got {tuple(q.shape)} / {tuple(k.shape)}")
    if key_mask is not None and not (key_mask.dtype == torch.uint8 and key_mask.is_contiguous() and tuple(key_mask.shape) == (B, S)):
        raise ValueError(f"{name}: key_mask must be contiguous uint8 [B, S]")


def qk_prepare_fwd(q, k, B, S, Hq, Hkv, D, key_mask=None, scale=None):
    """The prepared head-mean attention distribution of the causal softmax of ``scale * q k^T`` -> (P [B, S, S], Z [B, S], lse [B, Hq, S]).  Operands
    as ``kernels_llama.attn_max_logit`` takes them."""
    L.require_gpu(q, k, key_mask)
    _check_qk("ral qk_prepare_fwd", q, k, B, S, Hq, Hkv, D, key_mask)
    P = torch.empty((B, S, S), dtype=F32, device=q.device)
    Z = torch.empty((B, S), dtype=F32, device=q.device)
    lse = torch.empty((B, Hq, S), dtype=F32, device=q.device)
    scale = D ** -0.5 if scale is None else scale
    L.call("mi355_ral_qk_prepare_fwd", B, S, Hq, Hkv, D, L.ptr(q), _ld(q, Hq * D), L.ptr(k), _ld(k, Hkv * D), L.ptr(key_mask), scale, L.ptr(P), L.ptr(Z), L.ptr(lse))
    return P, Z, lse


def qk_prepare_bwd(q, k, da, lse, B, S, Hq, Hkv, D, key_mask=None, scale=None):
    """``da`` [B, S, S] (the gradient on the head mean; read strictly below the diagonal) -> (dq, dk) bf16, shaped like q and k."""
    L.require_gpu(q, k, da, lse, key_mask)
    _check_qk("ral qk_prepare_bwd", q, k, B, S, Hq, Hkv, D, key_mask)
    _f32(da, "ral qk_prepare_bwd: da", (B, S, S))
    _f32(lse, "ral qk_prepare_bwd: lse", (B, Hq, S))
    dq = torch.empty((B * S, Hq * D), dtype=BF16, device=q.device)
    dk = torch.empty((B * S, Hkv * D), dtype=BF16, device=q.device)
    delta = torch.empty((B, Hq, S), dtype=F32, device=q.device)
    scale = D ** -0.5 if scale is None else scale
    L.call("mi355_ral_qk_prepare_bwd", B, S, Hq, Hkv, D, L.ptr(q), _ld(q, Hq * D), L.ptr(k), _ld(k, Hkv * D), L.ptr(key_mask), scale, L.ptr(da), L.ptr(lse),
           L.ptr(delta), L.ptr(dq), Hq * D, L.ptr(dk), Hkv * D)
    return dq, dk


def _check_weights(name, w):
    if w.dim() != 4 or w.shape[2] != w.shape[3] or w.dtype not in (F32, BF16) or not w.is_contiguous() or w.shape[1] < 1:
        raise ValueError(f"{name}: attention weights must be contiguous fp32 / bf16 [b, heads, s, s], got {w.dtype} {tuple(w.shape)} strides {w.stride()}")


def prepare_fwd(weights):
    """Materialised attention weights [B, H, S, S] (fp32 or bf16) -> (P [B, S, S], Z [B, S])."""
    L.require_gpu(weights)
    _check_weights("ral prepare_fwd", weights)
    B, H, S, _ = weights.shape
    P = torch.empty((B, S, S), dtype=F32, device=weights.device)
    Z = torch.empty((B, S), dtype=F32, device=weights.device)
    L.call("mi355_ral_prepare_fwd", B, H, S, L.ptr(weights), L.dt_code(weights.dtype), L.ptr(P), L.ptr(Z))
    return P, Z


def prepare_bwd(da, H, dtype):
    """``da`` [B, S, S] -> dweights [B, H, S, S] of ``dtype``."""
    L.require_gpu(da)
    if da.dim() != 3:
        raise ValueError(f"ral prepare_bwd: da must be [B, S, S], got {tuple(da.shape)}")
    B, S, _ = da.shape
    _f32(da, "ral prepare_bwd: da", (B, S, S))
    if H < 1 or dtype not in (F32, BF16):
        raise ValueError(f"ral prepare_bwd: {H} heads of {dtype}")
    dw = torch.empty((B, H, S, S), dtype=dtype, device=da.device)
    L.call("mi355_ral_prepare_bwd", B, H, S, L.ptr(da), L.ptr(dw), L.dt_code(dtype))
    return dw


def renorm_bwd(P, Z, dP, causal):
    """dP -> da given P, Z; ``causal``: zero on and above the diagonal (the q, k path), else on the diagonal only."""
    L.require_gpu(P, Z, dP)
    if P.dim() != 3:
        raise ValueError(f"ral renorm_bwd: P must be [B, S, S], got {tuple(P.shape)}")
    B, S, _ = P.shape
    _f32(P, "ral renorm_bwd: P", (B, S, S))
    _f32(Z, "ral renorm_bwd: Z", (B, S))
    _f32(dP, "ral renorm_bwd: dP", (B, S, S))
    da = torch.empty_like(P)
    L.call("mi355_ral_renorm_bwd", B, S, L.ptr(P), L.ptr(Z), L.ptr(dP), int(bool(causal)), L.ptr(da))
    return da


def _check_pq(name, P, Q):
    if P.dim() != 3:
        raise ValueError(f"{name}: P must be [B, S, S], got {tuple(P.shape)}")
    B, S, _ = P.shape
    _f32(P, f"{name}: P", (B, S, S))
    _f32(Q, f"{name}: Q", (B, S, S))
    return B, S


def jsd_fwd(P, Q):
    """jsd [B, S] = 0.5 sum_j (P log(P / M) + Q log(Q / M))."""
    L.require_gpu(P, Q)
    B, S = _check_pq("ral jsd_fwd", P, Q)
    jsd = torch.empty((B, S), dtype=F32, device=P.device)
    L.call("mi355_ral_jsd_fwd", B, S, L.ptr(P), L.ptr(Q), L.ptr(jsd))
    return jsd


def jsd_bwd(P, Q, w):
    """dP = 0.5 w[b, i] log(P / M)."""
    L.require_gpu(P, Q, w)
    B, S = _check_pq("ral jsd_bwd", P, Q)
    _f32(w, "ral jsd_bwd: w", (B, S))
    dP = torch.empty_like(P)
    L.call("mi355_ral_jsd_bwd", B, S, L.ptr(P), L.ptr(Q), L.ptr(w), L.ptr(dP))
    return dP


def reduce(jsd, advantages, loss_mask, ral_factor=1.0, grad=None, want_loss=True, want_w=True):
    """-> (loss fp32 [] or None, w fp32 [B, S] or None): the advantage-weighted masked mean and the row weights of its backward, scaled by ``grad``
    (an fp32 scalar on the device; None: 1)."""
    L.require_gpu(jsd, advantages, loss_mask, grad)
    if jsd.dim() != 2 or jsd.shape[0] < 1 or jsd.shape[1] < 1:
        raise ValueError(f"ral reduce: jsd must be a non-empty [B, S], got {tuple(jsd.shape)}")
    B, S = jsd.shape
    _f32(jsd, "ral reduce: jsd", (B, S))
    _f32(advantages, "ral reduce: advantages", (B,))
    _f32(loss_mask, "ral reduce: loss_mask", (B, S))
    if grad is not None and (grad.dtype != F32 or grad.numel() != 1):
        raise ValueError(f"ral reduce: grad must be one fp32 value, got {grad.dtype} {tuple(grad.shape)}")
    if not (want_loss or want_w):
        raise ValueError("ral reduce: nothing to compute")
    loss = torch.empty((), dtype=F32, device=jsd.device) if want_loss else None
    w = torch.empty((B, S), dtype=F32, device=jsd.device) if want_w else None
    L.call("mi355_ral_reduce", B, S, L.ptr(jsd), L.ptr(advantages), L.ptr(loss_mask), float(ral_factor), L.ptr(grad), L.ptr(loss), L.ptr(w))
    return loss, w


def add_bf16_(dst, other):
    """dst = bf16(dst + other), both contiguous bf16 of one shape.  Returns dst."""
    L.require_gpu(dst, other)
    if dst.dtype != BF16 or other.dtype != BF16 or dst.shape != other.shape or not dst.is_contiguous() or not other.is_contiguous():
        raise ValueError(f"ral add_bf16: contiguous bf16 tensors of one shape expected, got {dst.dtype} {tuple(dst.shape)} and {other.dtype} {tuple(other.shape)}")
    L.call("mi355_ral_add_bf16", dst.numel(), L.ptr(dst), L.ptr(other), L.ptr(dst))
    return dst
