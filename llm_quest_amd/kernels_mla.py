"""Tensor-level launchers of the DeepSeek-V3 kernels (csrc/deepseek.hip): Multi-head Latent Attention and the decoupled RoPE; no autograd here.

Written like ``kernels_g3.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU, allocates its
outputs with torch (or takes them from the caller) and enqueues on torch's current stream.  There is no CPU fallback.

Notation: ``T = B * S`` tokens; ``Dn`` the head dim of q_nope / k_nope / v / o, ``Dr = Dn / 2`` the decoupled rotary dim.  Operands are
token-major bf16 with unit inner stride (row-strided views -- column slices of fused GEMM outputs -- allowed): q_nope / k_nope / v / o
``[T, Hq * Dn]``, q_rope ``[T, Hq * Dr]``, k_rope ``[T, Dr]``: one row per token, shared by all heads.
"""

import torch

from . import _lib as L

BF16, F32 = torch.bfloat16, torch.float32
DIM_PAIRS = ((64, 32), (128, 64))  # (Dn, Dr) the kernels are built for


def _operand(t, name, tokens, width):
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != tokens or t.shape[1] != width:
        raise ValueError(f"mla: {name} must be bf16 [tokens={tokens}, {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    if tokens > 1 and (t.stride(0) < width or t.stride(0) % 8):
        raise ValueError(f"mla: {name} row stride {t.stride(0)} must be a multiple of 8 and at least {width}")
    if t.data_ptr() % 16:
        raise ValueError(f"mla: {name} must be 16-byte aligned")


def _check(B, S, Hq, Dn, Dr):
    if B <= 0 or S <= 0 or Hq <= 0:
        raise ValueError(f"mla: batch, sequence length and heads must be positive, got ({B}, {S}, {Hq})")
    if (Dn, Dr) not in DIM_PAIRS:
        raise ValueError(f"mla: (head_dim, rope_dim) = ({Dn}, {Dr}) not built {DIM_PAIRS}")


def _ld(t):
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def mla_scale(Dn, Dr):
    return (Dn + Dr) ** -0.5


def mla_attn_fwd(q_nope, q_rope, k_nope, k_rope, v, B, S, Hq, Dn, Dr, scale=None, o=None):
    """Causal MLA attention.  Returns (o [B*S, Hq*Dn] bf16, lse fp32 [B, Hq, S])."""
    L.require_gpu(q_nope, q_rope, k_nope, k_rope, v, o)
    _check(B, S, Hq, Dn, Dr)
    T = B * S
    if o is None:
        o = torch.empty((T, Hq * Dn), dtype=BF16, device=q_nope.device)
    for t, n, w in ((q_nope, "q_nope", Hq * Dn), (q_rope, "q_rope", Hq * Dr), (k_nope, "k_nope", Hq * Dn), (k_rope, "k_rope", Dr), (v, "v", Hq * Dn), (o, "o", Hq * Dn)):
        _operand(t, n, T, w)
    lse = torch.empty((B, Hq, S), dtype=F32, device=q_nope.device)
    scale = mla_scale(Dn, Dr) if scale is None else scale
    L.call("mi355_mla_attn_fwd", B, S, Hq, Dn, Dr, L.ptr(q_nope), _ld(q_nope), L.ptr(q_rope), _ld(q_rope), L.ptr(k_nope), _ld(k_nope), L.ptr(k_rope), _ld(k_rope),
           L.ptr(v), _ld(v), L.ptr(o), _ld(o), L.ptr(lse), scale)
    return o, lse


def mla_attn_bwd(q_nope, q_rope, k_nope, k_rope, v, o, do, lse, B, S, Hq, Dn, Dr, dq_nope=None, dq_rope=None, dk_nope=None, dv=None, dk_rope_heads=None, scale=None):
    """dq_nope / dq_rope / dk_nope / dv: caller-provided (possibly row-strided) destinations, or new tensors.  The gradient of the shared key
    comes back PER HEAD, fp32 ``[B*S, Hq, Dr]``: ``mla_rope_bwd`` sums it over heads.  Returns (dq_nope, dq_rope, dk_nope, dk_rope_heads, dv)."""
    L.require_gpu(q_nope, q_rope, k_nope, k_rope, v, o, do, lse, dq_nope, dq_rope, dk_nope, dv, dk_rope_heads)
    _check(B, S, Hq, Dn, Dr)
    dev, T = q_nope.device, B * S
    new = lambda w: torch.empty((T, w), dtype=BF16, device=dev)
    dq_nope = new(Hq * Dn) if dq_nope is None else dq_nope
    dq_rope = new(Hq * Dr) if dq_rope is None else dq_rope
    dk_nope = new(Hq * Dn) if dk_nope is None else dk_nope
    dv = new(Hq * Dn) if dv is None else dv
    if dk_rope_heads is None:
        dk_rope_heads = torch.empty((T, Hq, Dr), dtype=F32, device=dev)
    for t, n, w in ((q_nope, "q_nope", Hq * Dn), (q_rope, "q_rope", Hq * Dr), (k_nope, "k_nope", Hq * Dn), (k_rope, "k_rope", Dr), (v, "v", Hq * Dn), (o, "o", Hq * Dn),
                    (do, "do", Hq * Dn), (dq_nope, "dq_nope", Hq * Dn), (dq_rope, "dq_rope", Hq * Dr), (dk_nope, "dk_nope", Hq * Dn), (dv, "dv", Hq * Dn)):
        _operand(t, n, T, w)
    if not (lse.dtype == F32 and lse.is_contiguous() and tuple(lse.shape) == (B, Hq, S)):
        raise ValueError("mla: lse must be contiguous fp32 [B, Hq, S]")
    if not (dk_rope_heads.dtype == F32 and dk_rope_heads.is_contiguous() and tuple(dk_rope_heads.shape) == (T, Hq, Dr) and dk_rope_heads.data_ptr() % 16 == 0):
        raise ValueError(f"mla: dk_rope_heads must be contiguous 16-byte aligned fp32 [{T}, {Hq}, {Dr}]")
    delta = torch.empty_like(lse)
    scale = mla_scale(Dn, Dr) if scale is None else scale
    L.call("mi355_mla_attn_bwd", B, S, Hq, Dn, Dr, L.ptr(q_nope), _ld(q_nope), L.ptr(q_rope), _ld(q_rope), L.ptr(k_nope), _ld(k_nope), L.ptr(k_rope), _ld(k_rope),
           L.ptr(v), _ld(v), L.ptr(o), _ld(o), L.ptr(do), _ld(do), L.ptr(lse), L.ptr(delta), L.ptr(dq_nope), _ld(dq_nope), L.ptr(dq_rope), _ld(dq_rope),
           L.ptr(dk_nope), _ld(dk_nope), L.ptr(dk_rope_heads), L.ptr(dv), _ld(dv), scale)
    return dq_nope, dq_rope, dk_nope, dk_rope_heads, dv


def _rope_rows(t, name, tokens, width):
    if t.dtype != BF16 or t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != tokens or t.shape[1] != width or (tokens > 1 and t.stride(0) < width):
        raise ValueError(f"mla rope: {name} must be bf16 [tokens={tokens}, {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")


def _check_rope(T, S, Hq, Dr, cos, sin):
    if Dr not in (32, 64):
        raise ValueError(f"mla rope: rope_dim {Dr} not built (32, 64)")
    if T <= 0 or S <= 0 or Hq <= 0 or T % S:
        raise ValueError(f"mla rope: {T} tokens must be a positive multiple of the sequence length {S}; heads {Hq} positive")
    for t, n in ((cos, "cos"), (sin, "sin")):
        if t.dtype != F32 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != Dr or t.shape[0] < S:
            raise ValueError(f"mla rope: {n} must be contiguous fp32 [>= {S}, {Dr}], got {t.dtype} {tuple(t.shape)}")


def mla_rope_fwd(q_rope_pre, k_rope_pre, S, Hq, Dr, cos, sin, q_rope=None, k_rope=None):
    """Half-split rotation of the q_rope heads [T, Hq*Dr] and of the shared key [T, Dr] (both possibly row-strided); position = token % S.
    Returns (q_rope, k_rope) bf16."""
    L.require_gpu(q_rope_pre, k_rope_pre, cos, sin, q_rope, k_rope)
    T = q_rope_pre.shape[0]
    _check_rope(T, S, Hq, Dr, cos, sin)
    dev = q_rope_pre.device
    q_rope = torch.empty((T, Hq * Dr), dtype=BF16, device=dev) if q_rope is None else q_rope
    k_rope = torch.empty((T, Dr), dtype=BF16, device=dev) if k_rope is None else k_rope
    for t, n, w in ((q_rope_pre, "q_rope_pre", Hq * Dr), (k_rope_pre, "k_rope_pre", Dr), (q_rope, "q_rope", Hq * Dr), (k_rope, "k_rope", Dr)):
        _rope_rows(t, n, T, w)
    L.call("mi355_mla_rope_fwd", T, S, Hq, Dr, L.ptr(q_rope_pre), _ld(q_rope_pre), L.ptr(k_rope_pre), _ld(k_rope_pre), L.ptr(cos), L.ptr(sin), cos.shape[0],
           L.ptr(q_rope), _ld(q_rope), L.ptr(k_rope), _ld(k_rope))
    return q_rope, k_rope


def mla_rope_bwd(dq_rope, dk_rope_heads, S, Hq, Dr, cos, sin, dq_rope_pre=None, dk_rope_pre=None):
    """The adjoint rotation.  ``dk_rope_heads`` fp32 [T, Hq, Dr] is summed over heads 0 .. Hq-1 in that order first.  Returns
    (dq_rope_pre [T, Hq*Dr], dk_rope_pre [T, Dr]) bf16; both may be row-strided destinations."""
    L.require_gpu(dq_rope, dk_rope_heads, cos, sin, dq_rope_pre, dk_rope_pre)
    T = dq_rope.shape[0]
    _check_rope(T, S, Hq, Dr, cos, sin)
    dev = dq_rope.device
    dq_rope_pre = torch.empty((T, Hq * Dr), dtype=BF16, device=dev) if dq_rope_pre is None else dq_rope_pre
    dk_rope_pre = torch.empty((T, Dr), dtype=BF16, device=dev) if dk_rope_pre is None else dk_rope_pre
    for t, n, w in ((dq_rope, "dq_rope", Hq * Dr), (dq_rope_pre, "dq_rope_pre", Hq * Dr), (dk_rope_pre, "dk_rope_pre", Dr)):
        _rope_rows(t, n, T, w)
    if not (dk_rope_heads.dtype == F32 and dk_rope_heads.is_contiguous() and tuple(dk_rope_heads.shape) == (T, Hq, Dr)):
        raise ValueError(f"mla rope: dk_rope_heads must be contiguous fp32 [{T}, {Hq}, {Dr}]")
    L.call("mi355_mla_rope_bwd", T, S, Hq, Dr, L.ptr(dq_rope), _ld(dq_rope), L.ptr(dk_rope_heads), L.ptr(cos), L.ptr(sin), cos.shape[0],
           L.ptr(dq_rope_pre), _ld(dq_rope_pre), L.ptr(dk_rope_pre), _ld(dk_rope_pre))
    return dq_rope_pre, dk_rope_pre
