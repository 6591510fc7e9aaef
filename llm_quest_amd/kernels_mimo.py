"""Tensor-level launchers of the MiMo-V2-Flash kernels (sink attention: csrc/attention_band.hip; norm + RoPE: csrc/mimo.hip); no autograd here.

Written like ``kernels_g3.py``: every launcher checks shapes / strides / dtypes on the host before a pointer reaches the GPU, allocates its
outputs with torch and enqueues on torch's current stream.  There is no CPU fallback.

Notation: ``T = B * S`` tokens; attention operands are token-major bf16 with unit inner stride (row-strided views allowed): q ``[T, Hq * D]``,
k ``[T, Hkv * D]``, v ``[T, Hkv * DV]``, o ``[T, Hq * DV]``; ``W`` is the window: key j is visible to query i iff ``i - W < j <= i``;
``sink`` is one logit per query head (bf16 or fp32 ``[Hq]``) that enters the softmax denominator only, or None.
"""

import torch

from . import _lib as L
from . import kernels as K
from . import kernels_g3 as KG
from .kernels_g3 import _ld

BF16, F32 = torch.bfloat16, torch.float32
MIMO_PARTS = 512  # max workgroups (= rows of partials) of the backwards that reduce parameter gradients
HEAD_DIM_PAIRS = ((64, 32), (64, 64), (128, 64), (128, 128), (192, 128))  # (head_dim, value_head_dim)
NORM_HEAD_DIMS = (64, 128, 192)
RMS_EPS = 1e-6
WHO = "sink attention"  # the family label in the error texts of the attention host checks, which are kernels_g3's


def _pair_error(D, DV):
    return None if (D, DV) in HEAD_DIM_PAIRS else f"(head_dim, value_head_dim) = ({D}, {DV}) not built {HEAD_DIM_PAIRS}"


def check_pair(D, DV, what="sink attention"):
    if _pair_error(D, DV):
        raise ValueError(f"{what}: {_pair_error(D, DV)}")


def _sink_f32(sink, Hq):
    """The sink logits as the kernels take them: contiguous fp32 [Hq] (a bf16 parameter casts up losslessly), or None."""
    if sink is None:
        return None
    if sink.dtype not in (BF16, F32) or sink.dim() != 1 or sink.shape[0] != Hq:
        raise ValueError(f"sink attention: sink must be bf16 or fp32 [{Hq}], got {sink.dtype} {tuple(sink.shape)}")
    sink = sink.detach()
    return sink.contiguous() if sink.dtype == F32 else K.cast(sink.contiguous(), F32)


def sink_attn_fwd(q, k, v, B, S, Hq, Hkv, D, DV, W, sink=None, scale=None):
    """Causal / sliding-window attention with an optional sink.  Returns (o [B*S, Hq*DV] bf16, lse fp32 [B, Hq, S], the sink included)."""
    L.require_gpu(q, k, v, sink)
    KG._check_attn(WHO, B, S, Hq, Hkv, W, _pair_error(D, DV))
    KG._fwd_operands(WHO, q, k, v, B, S, Hq, Hkv, D, DV)
    z = _sink_f32(sink, Hq)
    o = torch.empty((B * S, Hq * DV), dtype=BF16, device=q.device)
    lse = torch.empty((B, Hq, S), dtype=F32, device=q.device)
    scale = D ** -0.5 if scale is None else scale
    L.require_gpu(q, k, v, z)
    L.call("mi355_sink_attn_fwd", B, S, Hq, Hkv, D, DV, min(int(W), 2**31 - 1), L.ptr(q), _ld(q), L.ptr(k), _ld(k), L.ptr(v), _ld(v), L.ptr(z), L.ptr(o), Hq * DV,
           L.ptr(lse), scale)
    return o, lse


def sink_attn_bwd(q, k, v, o, do, lse, B, S, Hq, Hkv, D, DV, W, sink=None, dq=None, dk=None, dv=None, scale=None, parts=None):
    """dq / dk / dv: caller-provided (possibly row-strided) destinations, or new tensors.  Returns (dq, dk, dv, dsink): dsink fp32 [Hq]
    (per-workgroup partial rows folded in a fixed order), None without a sink."""
    L.require_gpu(q, k, v, o, do, lse, dq, dk, dv, sink)
    KG._check_attn(WHO, B, S, Hq, Hkv, W, _pair_error(D, DV))
    dq, dk, dv = KG._bwd_operands(WHO, q, k, v, o, do, lse, dq, dk, dv, B, S, Hq, Hkv, D, DV)
    z = _sink_f32(sink, Hq)
    delta = torch.empty_like(lse)
    scale = D ** -0.5 if scale is None else scale
    part = None
    if z is not None:
        parts = min(MIMO_PARTS, max(1, (B * S + 255) // 256)) if parts is None else parts
        if parts < 1:
            raise ValueError(f"sink attention: parts must be positive, got {parts}")
        part = (torch.zeros if B * S == 0 else torch.empty)((parts, Hq), dtype=F32, device=q.device)
    L.require_gpu(q, k, v, o, do, lse, dq, dk, dv, z)
    L.call("mi355_sink_attn_bwd", B, S, Hq, Hkv, D, DV, min(int(W), 2**31 - 1), L.ptr(q), _ld(q), L.ptr(k), _ld(k), L.ptr(v), _ld(v), L.ptr(o), _ld(o), L.ptr(do),
           _ld(do), L.ptr(z), L.ptr(lse), L.ptr(delta), L.ptr(dq), _ld(dq), L.ptr(dk), _ld(dk), L.ptr(dv), _ld(dv), L.ptr(part), 0 if part is None else parts, scale)
    return dq, dk, dv, (None if part is None else L.reduce_rows(part))


def _vec(t, name, n):
    if t.dtype != BF16 or not t.is_contiguous() or t.numel() != n:
        raise ValueError(f"{name}: expected contiguous bf16 with {n} elements, got {t.dtype} {tuple(t.shape)}")


def _check_normrope(name, x, S, Hq, Hkv, D, cos, sin, q_weight, k_weight):
    if D not in NORM_HEAD_DIMS:
        raise ValueError(f"{name}: head_dim {D} not built {NORM_HEAD_DIMS}")
    if Hq < 0 or Hkv < 0 or Hq + Hkv == 0 or S <= 0:
        raise ValueError(f"{name}: bad head counts / sequence length ({Hq}, {Hkv}, {S})")
    width = (Hq + Hkv) * D
    if x.dim() != 2 or x.dtype != BF16 or x.stride(1) != 1 or x.shape[1] < width or (x.shape[0] > 1 and x.stride(0) < width):
        raise ValueError(f"{name}: expected bf16 [tokens, >= {width}] with unit inner stride, got {x.dtype} {tuple(x.shape)} {x.stride()}")
    if x.shape[0] % S:
        raise ValueError(f"{name}: {x.shape[0]} tokens are no multiple of the sequence length {S}")
    if cos.dim() != 2 or tuple(cos.shape) != tuple(sin.shape):
        raise ValueError(f"{name}: cos and sin must be [rows, R] tables of one shape, got {tuple(cos.shape)} and {tuple(sin.shape)}")
    R = cos.shape[1]
    if R < 2 or R > D or R % 2:
        raise ValueError(f"{name}: the rotated width {R} (the tables' width) must be even and in [2, head_dim = {D}]")
    for t, n in ((cos, "cos"), (sin, "sin")):
        if t.dtype != F32 or not t.is_contiguous() or t.shape[0] < S:
            raise ValueError(f"{name}: {n} must be contiguous fp32 [>= {S}, {R}], got {t.dtype} {tuple(t.shape)}")
    _vec(q_weight, f"{name}: q_weight", D)
    _vec(k_weight, f"{name}: k_weight", D)
    return R


def normrope_fwd(x, S, Hq, Hkv, D, cos, sin, q_weight, k_weight, eps=RMS_EPS):
    """Per-head RMSNorm then partial RoPE on the q and k heads of x [T, >= (Hq+Hkv)*D] (q heads first; further columns, the v heads of a fused
    projection, are not touched).  The tables' width R is the rotated width.  Returns y [T, (Hq+Hkv)*D] bf16."""
    L.require_gpu(x, cos, sin, q_weight, k_weight)
    R = _check_normrope("mimo normrope_fwd", x, S, Hq, Hkv, D, cos, sin, q_weight, k_weight)
    T, width = x.shape[0], (Hq + Hkv) * D
    y = torch.empty((T, width), dtype=BF16, device=x.device)
    L.call("mi355_mimo_normrope_fwd", T, S, Hq, Hkv, D, R, L.ptr(x), max(x.stride(0), width), L.ptr(q_weight), L.ptr(k_weight), L.ptr(cos), L.ptr(sin), cos.shape[0],
           L.ptr(y), width, eps)
    return y


def normrope_bwd(x, dy, S, Hq, Hkv, D, cos, sin, q_weight, k_weight, dx=None, eps=RMS_EPS, parts=None):
    """-> (dx, dq_weight, dk_weight): dx bf16 like the q / k columns of x (``dx`` may be a row-strided destination, the gradient of a fused
    projection, whose further columns stay as they are), the two weight gradients fp32 [D] views of one reduced row."""
    L.require_gpu(x, dy, cos, sin, dx, q_weight, k_weight)
    R = _check_normrope("mimo normrope_bwd", x, S, Hq, Hkv, D, cos, sin, q_weight, k_weight)
    T, width = x.shape[0], (Hq + Hkv) * D
    if T == 0:
        raise ValueError("mimo normrope_bwd: no tokens")
    if dx is None:
        dx = torch.empty((T, width), dtype=BF16, device=x.device)
    for t, n in ((dy, "dy"), (dx, "dx")):
        if t.dim() != 2 or t.dtype != BF16 or t.stride(1) != 1 or t.shape[0] != T or t.shape[1] < width or (T > 1 and t.stride(0) < width):
            raise ValueError(f"mimo normrope_bwd: {n} must be bf16 [{T}, >= {width}] with unit inner stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    parts = min(MIMO_PARTS, (T * (Hq + Hkv) + 3) // 4) if parts is None else parts
    if parts < 1:
        raise ValueError(f"mimo normrope_bwd: parts must be positive, got {parts}")
    part = torch.empty((parts, 2 * D), dtype=F32, device=x.device)
    L.call("mi355_mimo_normrope_bwd", T, S, Hq, Hkv, D, R, L.ptr(x), max(x.stride(0), width), L.ptr(q_weight), L.ptr(k_weight), L.ptr(cos), L.ptr(sin), cos.shape[0],
           L.ptr(dy), max(dy.stride(0), width), L.ptr(dx), max(dx.stride(0), width), L.ptr(part), parts, eps)
    row = L.reduce_rows(part)
    return dx, row[:D], row[D:]
